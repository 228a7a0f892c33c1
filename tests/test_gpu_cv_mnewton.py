"""Cross-validation in multinomial Newton mode: every fold fit of every alpha from ONE native call whose jobs advance in
lock-step (sa.cv_mnewton_fits -> sgdnet_cv_mnewton_*, sgdnet_amd/csrc/mnewton.hip: mnewton_cv_run) and sa.cv_sgdnet_mnewton
on top of it.

Fold fit (alpha, fold j) is BY DEFINITION sa.sgdnet_mnewton(x[T], y[T], alpha=alpha, lambda_=lambda) for the training set T
of fold j.  The primary check is independent of any solver: the optimality conditions of that problem on x[T], y[T] (sa.kkt)
within the project's bound, for every job and every lambda, for the coefficients and for the class-centred intercepts.  The
second check is the separate fit itself, to the project's figure for "the same optimum reached twice".

Tolerances
  KKT_BOUND = 1e-8          KKT residual <= 1e-8 * lambda, coefficients and intercepts: tests/test_gpu_mnewton.py.
  SAME_OPTIMUM = 1e-9       coefficients relative to max|beta|, class-centred intercepts relative to max(1, max|a0|), dev_ratio
                            relative.  Both fits stop at thresh = 1e-12; tests/test_cv_mnewton_host.py measures what centres
                            formed on the host instead of the device cost at that thresh (CENTRE_BOUND <= 1e-10, so the
                            project's 1e-9 of tests/test_gpu_cv_covariance.py stands: tests/cv_mnewton_reference.py).
At mix = 1 and an even K the optimum is not unique in the coefficients (tests/test_gpu_mnewton.py): there the certificate and
dev_ratio are compared -- a condition on the parameters, never on the data.

The shapes (n, p, K, folds) are tests/cv_mnewton_reference.py's, with what each straddles.  The lambdas are the driver's
automatic path of the whole data (tm.automatic_lambdas), handed to every job as user lambdas.  Every fold helper asserts
that every training set holds every class (ref.folds): the seeds were picked on the CPU so that they do."""
import numpy as np
import pytest
import scipy.sparse as sp

import cv_mnewton_reference as ref
import test_gpu_cv_covariance as tcv
import test_gpu_mnewton as tm
import test_gpu_newton as tn

pytestmark = pytest.mark.gpu

KKT_BOUND = tm.KKT_BOUND
SAME_OPTIMUM = ref.SAME_OPTIMUM
SHAPES, LIMIT_SHAPES, MIXES, NLAMBDA, THRESH = ref.SHAPES, ref.LIMIT_SHAPES, ref.MIXES, ref.NLAMBDA, ref.THRESH
assert KKT_BOUND == tn.KKT_BOUND == 1e-8 and SAME_OPTIMUM == tcv.SAME_OPTIMUM

training_sets, assert_optimal, rows, stacked = tcv.training_sets, tm.assert_optimal, ref.rows, tm.stacked


@pytest.fixture(scope="module")
def sa():
    import torch  # noqa: F401
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    return sgdnet_amd


def assert_same_fit(got, ref_fit, what, coefficients):
    d = np.abs(got.dev_ratio - ref_fit.dev_ratio).max() / np.abs(ref_fit.dev_ratio).max()
    b = a = 0.0
    if coefficients:
        b = np.abs(stacked(got) - stacked(ref_fit)).max() / np.abs(stacked(ref_fit)).max()
        a = np.abs(got.a0 - ref_fit.a0).max() / max(1.0, np.abs(ref_fit.a0).max())
    print(what, "vs the separate fit: beta %.3g dev_ratio %.3g a0 %.3g" % (b, d, a))
    assert b <= SAME_OPTIMUM and d <= SAME_OPTIMUM and a <= SAME_OPTIMUM, (what, b, d, a)
    assert got.nobs == ref_fit.nobs and abs(got.nulldev - ref_fit.nulldev) <= SAME_OPTIMUM * ref_fit.nulldev


def check_jobs(sa, x, y, K, foldid, mixes, train_on, standardize=True, intercept=True, compare=True, nlambda=NLAMBDA, lambda_min_ratio=1e-2,
               lam=None):
    """one batched call over `mixes`; KKT on x[T], y[T] for every job and lambda, and the separate fit of every job"""
    ref.folds(foldid, y, K)
    opts = dict(standardize=standardize, intercept=intercept, thresh=THRESH)
    if lam is None:
        lam = [ref.lambdas(x, y, K, m, standardize, nlambda, lambda_min_ratio) for m in mixes]
    fits = sa.cv_mnewton_fits(x, y, foldid, mixes, lam, train_on=train_on, **opts)
    sets = training_sets(foldid, train_on)
    assert len(fits) == len(mixes) * len(sets)
    p = x.shape[1]
    for a, m in enumerate(mixes):
        for j, T in enumerate(sets):
            fit, xT, yT = fits[a * len(sets) + j], rows(x, T), y[T]
            what = (x.shape, K, sp.issparse(x), m, train_on, standardize, intercept, j)
            assert (fit.return_codes == 0).all() and fit.draws_used == 0 and fit.alpha == m and fit.family == "multinomial", what
            assert np.array_equal(fit.lambda_, lam[a]) and np.isfinite(fit.dev_ratio).all() and fit.nobs == T.sum(), what
            assert fit.classnames == [str(v) for v in np.unique(y)] and fit.grouped is False, what
            assert fit.a0.shape == (K, len(lam[a])) and len(fit.beta) == K and all(b.shape == (p, len(lam[a])) for b in fit.beta), what
            assert fit.dfmat.shape == (K, len(lam[a])), what
            assert fit.npasses == 1 + fit.diagnostics["steps"] + fit.diagnostics["halvings"] and fit.diagnostics["steps"] >= len(lam[a]), what
            assert_optimal(sa.kkt(fit, xT, yT, standardize=standardize, intercept=intercept), fit.lambda_, what)     # no job, no lambda dropped
            if compare:
                sep = sa.sgdnet_mnewton(xT, yT, alpha=m, lambda_=lam[a], **opts)
                assert_same_fit(fit, sep, what, ref.coefficients_are_unique(m, K))
    return fits


# ---- 1. the envelope ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_fold_fit_is_optimal_and_the_separate_fit(sa, shape, sparse, train_on):
    n, p, K, G = shape
    x, y = tm.problem(n, p, K, sparse)
    check_jobs(sa, x, y, K, tcv.equal_folds(n, G), MIXES, train_on)


@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", LIMIT_SHAPES)
def test_every_fold_fit_at_the_feature_limit_is_optimal(sa, shape, sparse, train_on):
    """one workgroup's LDS at the limit: one mix per case, rotated so that the four cases of a shape see all three; KKT only"""
    n, K, G = shape[0], shape[2], shape[3]
    p = tm.pmax(K)
    assert K * (p + 1) == 198
    x, y = tm.problem(n, p, K, sparse)
    mix = MIXES[(2 * sparse + (train_on == "rest") + 1) % 3]
    check_jobs(sa, x, y, K, tcv.equal_folds(n, G), [mix], train_on, compare=False, nlambda=4, lambda_min_ratio=tm.ratio_for((n, None, K)))


# ---- 2. intercept x standardize ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]])
def test_intercept_and_standardize_combinations(sa, shape, sparse, train_on):
    n, p, K, G = shape
    x, y = tm.problem(n, p, K, sparse, seed=1)
    for intercept, standardize in ((True, False), (False, True), (False, False)):     # (True, True) is the test above
        check_jobs(sa, x, y, K, tcv.equal_folds(n, G, seed=3), MIXES, train_on, standardize=standardize, intercept=intercept)


# ---- 3. awkward folds ----

@pytest.mark.parametrize("sparse", [False, True])
def test_folds_cut_along_a_sorted_column(sa, sparse):
    """every fold's mean of column 0 sits far from the whole-data mean the per-group sums are taken about"""
    n, p, K, G = 195, 14, 3, 3
    x, y = tm.problem(n, p, K, sparse, seed=2)
    col = np.asarray(x[:, 0].todense()).ravel() if sparse else x[:, 0]
    foldid = np.empty(n, dtype=np.int64)
    foldid[np.argsort(col, kind="stable")] = np.arange(n) * G // n
    for train_on in ("fold", "rest"):
        check_jobs(sa, x, y, K, foldid, [0.5, 1.0], train_on)


@pytest.mark.parametrize("sparse", [False, True])
def test_unequal_groups_with_arbitrary_labels(sa, sparse):
    n, p, K = 150, 5, 3
    x, y = tm.problem(n, p, K, sparse, seed=3)
    foldid = np.repeat([10, 20, 30, 40], [12, 38, 65, 35])         # labels need not be 1..G; a group of twelve rows
    foldid = foldid[np.random.default_rng(4).permutation(n)]
    for train_on in ("fold", "rest"):
        check_jobs(sa, x, y, K, foldid, [0.5, 1.0], train_on)


@pytest.mark.parametrize("sparse", [False, True])
def test_leave_one_out(sa, sparse):
    """n = 12, p = 2, K = 3, four rows per class: every complement of one row holds every class"""
    n, p, K = 12, 2, 3
    x, _ = tm.problem(n, p, K, sparse, seed=4)
    y = np.repeat(np.arange(K), 4).astype(float)[np.random.default_rng(4).permutation(n)]
    foldid = np.arange(n)
    assert all(np.bincount(y[T].astype(int), minlength=K).min() > 0 for T in training_sets(foldid, "rest"))
    opts = dict(thresh=THRESH)
    lam = [ref.lambdas(x, y, K, m) for m in (0.5, 1.0)]
    fits = sa.cv_mnewton_fits(x, y, foldid, [0.5, 1.0], lam, train_on="rest", **opts)           # nfolds = n
    assert len(fits) == 2 * n
    for a, m in enumerate((0.5, 1.0)):
        for j, T in enumerate(training_sets(foldid, "rest")):
            fit, what = fits[a * n + j], ("leave one out", sparse, m, j)
            assert (fit.return_codes == 0).all() and fit.nobs == n - 1, what
            assert_optimal(sa.kkt(fit, rows(x, T), y[T]), fit.lambda_, what)
            assert_same_fit(fit, sa.sgdnet_mnewton(rows(x, T), y[T], alpha=m, lambda_=lam[a], **opts), what, True)


@pytest.mark.parametrize("sparse", [False, True])
def test_large_mean_column(sa, sparse):
    """a column of mean 1e6 and sd 1 (every entry stored): KKT on x[T], y[T] only, on the path of
    tests/test_gpu_cv_newton.py::test_large_mean_column (10 lambdas, lambda_min_ratio = 0.05) for the reason given there"""
    n, p, K, G = 195, 5, 3, 3
    x, _ = tm.problem(n, p, K, sparse, seed=5)
    xd = np.asarray(x.todense()) if sparse else x.copy()
    rng = np.random.default_rng(11)
    col = rng.standard_normal(n)
    col = (col - col.mean()) / col.std()
    xd[:, 2] = 1e6 + col
    eta = np.column_stack([0.4 * (xd[:, 0] - xd[:, 0].mean()) + 0.7 * col, -0.7 * col, np.zeros(n)])
    pr = np.exp(eta - eta.max(axis=1, keepdims=True))
    pr /= pr.sum(axis=1, keepdims=True)
    y = (pr.cumsum(axis=1) < rng.random(n)[:, None]).sum(axis=1).clip(0, K - 1).astype(float)
    x = sp.csc_matrix(xd) if sparse else xd
    for train_on in ("fold", "rest"):
        check_jobs(sa, x, y, K, tcv.equal_folds(n, G, seed=5), [0.5, 1.0], train_on, compare=False, nlambda=10, lambda_min_ratio=0.05)


# ---- 4. jobs at different lambdas in one round ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
def test_jobs_progress_at_their_own_pace(sa, sparse, train_on):
    x, y = ref.steep_problem(sparse)
    S = ref.STEEP
    fits = check_jobs(sa, x, y, S["K"], tcv.equal_folds(S["n"], S["folds"], seed=S["fold_seed"]), S["mixes"], train_on, compare=False,
                      lam=[np.array(ref.STEEP_LAMBDAS)] * len(S["mixes"]))
    steps = [f.diagnostics["steps"] for f in fits]
    print("steps per job", steps, "halvings per job", [f.diagnostics["halvings"] for f in fits])
    # the jobs need different numbers of steps: the lock-step loop ran jobs at different lambdas in the same round
    assert len(set(steps)) > 1, steps


# ---- 5. independence and determinism ----

def test_jobs_are_independent_and_repeatable(sa):
    n, p, K, G = SHAPES[5]
    assert (n, p, K, G) == (1003, 6, 4, 10)
    xs, y = tm.problem(n, p, K, True, seed=6)
    xd = np.asarray(xs.todense())
    foldid = ref.equal_folds(n, G, y, K, seed=6)
    lam = np.geomspace(0.1, 0.002, 6)
    kw = dict(thresh=1e-9)
    alone = sa.cv_mnewton_fits(xd, y, foldid, [0.5], [lam], **kw)
    among = sa.cv_mnewton_fits(xd, y, foldid, [0.2, 0.5, 1.0], [lam, lam, lam], **kw)
    again = sa.cv_mnewton_fits(xd, y, foldid, [0.2, 0.5, 1.0], [lam, lam, lam], **kw)
    sparse = sa.cv_mnewton_fits(sp.csc_matrix(xs), y, foldid, [0.2, 0.5, 1.0], [lam, lam, lam], **kw)

    def same(f, g, what):
        assert stacked(f).tobytes() == stacked(g).tobytes(), (what, "beta")
        for name in ("a0", "dev_ratio", "return_codes"):
            assert getattr(f, name).tobytes() == getattr(g, name).tobytes(), (what, name)
        assert f.npasses == g.npasses > 0 and f.diagnostics["steps"] == g.diagnostics["steps"] > 0 and f.nulldev == g.nulldev, what

    for j in range(G):
        same(alone[j], among[G + j], ("alone / among", j))
    for j, (f, g, h) in enumerate(zip(among, again, sparse)):
        same(f, g, ("again", j))
        same(f, h, ("sparse / dense", j))


# ---- 6. cv_sgdnet_mnewton on iris ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
def test_cv_sgdnet_mnewton_batched_is_the_separate_cv_on_iris(sa, train_on):
    x, y = tm.iris()
    kw = dict(alpha=[0.5, 1], nfolds=5, seed=1, train_on=train_on, thresh=THRESH, nlambda=20)
    sep = sa.cv_sgdnet_mnewton(x, y, fold_fits="separate", **kw)
    bat = sa.cv_sgdnet_mnewton(x, y, fold_fits="batched", **kw)
    ref.folds(bat.foldid, y, 3)
    assert np.array_equal(sep.foldid, bat.foldid) and sep.name == bat.name == "Multnomial Deviance"
    assert sep.cv_summary.shape == bat.cv_summary.shape and np.array_equal(sep.cv_summary[:, :2], bat.cv_summary[:, :2])
    for a, b in zip(sep.lambda_, bat.lambda_):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(sep.cv_raw, bat.cv_raw):
        err = np.abs(a - b).max() / np.abs(a).max()
        print("iris %s: cv_raw batched vs separate, relative %.3g" % (train_on, err))
        assert err <= SAME_OPTIMUM
    assert (sep.alpha_min, sep.lambda_min, sep.lambda_1se) == (bat.alpha_min, bat.lambda_min, bat.lambda_1se)
    whole = sa.sgdnet_mnewton(x, y, alpha=bat.fit.alpha, nlambda=20, thresh=THRESH)
    for fit in (sep.fit, bat.fit):
        assert stacked(fit).tobytes() == stacked(whole).tobytes() and fit.a0.tobytes() == whole.a0.tobytes() and fit.draws_used == 0


@pytest.mark.parametrize("type_measure", ["deviance", "class"])
def test_generator_ends_in_the_same_state(sa, type_measure):
    x, y = tm.iris()
    state, folds = [], []
    for fold_fits in ("separate", "batched"):
        rng = sa.RRng(3)
        cv = sa.cv_sgdnet_mnewton(x, y, alpha=[0.5, 1.0], nfolds=3, rng=rng, nlambda=5, type_measure=type_measure, fold_fits=fold_fits)
        state.append(bytes(rng.state))
        folds.append(cv.foldid)
    ref.folds(folds[1], y, 3)
    assert state[0] == state[1] and state[0] != bytes(sa.RRng(3).state)       # (sample() for the fold ids moved it)
    assert np.array_equal(folds[0], folds[1])
    rng = sa.RRng(3)                                                           # ... and nothing else did
    rng.sample(x.shape[0])
    assert state[0] == bytes(rng.state)


# ---- 7. refusals ----

def test_refusals_name_the_condition(sa):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    score = x[:, 0] + rng.standard_normal(60)
    cls3 = np.digitize(score, [-0.5, 0.5]).astype(float)
    cls2 = (score > 0).astype(float)
    fold = np.arange(60) % 3

    def refused(code, needle, xx, yy, ff, alpha=0.5, **kw):
        with pytest.raises(sa.SgdnetError) as e:
            sa.cv_mnewton_fits(xx, yy, ff, alpha, [[0.1, 0.01]] * np.size(alpha) if np.ndim(alpha) else [0.1, 0.01], **kw)
        assert e.value.code == code and needle in str(e.value), str(e.value)

    wide = rng.standard_normal((30, sa.mnewton_max_features(3) + 1))
    refused(-5, "mode = mnewton needs no more features than sgdnet_mnewton_max_features(n_classes)", wide, np.arange(30) % 3, np.arange(30) // 10)
    refused(-5, "mode = mnewton needs no more features", sp.csc_matrix(wide), np.arange(30) % 3, np.arange(30) // 10)
    missing = fold.copy()
    order = np.argsort(cls3, kind="stable")
    first = int((cls3 == 0).sum())
    missing[order[:first]] = 0                                       # group 0: the rows of class 0 and nothing else
    missing[order[first:]] = 1 + np.arange(60 - first) % 2
    refused(-1, "the training set of group 0 of 3 holds no row of class 1", x, cls3, missing)
    # sgdnet(), cv_sgdnet() and the binomial Newton CV are as they were
    with pytest.raises(ValueError, match="mode must be one of 'exact', 'batched', 'auto', 'covariance'$"):
        sa.sgdnet(x, cls3, family="multinomial", nlambda=3, mode="mnewton")
    with pytest.raises(ValueError, match="mode must be one of"):
        sa.cv_sgdnet(x, cls3, family="multinomial", nfolds=3, nlambda=3, mode="mnewton")
    with pytest.raises(ValueError, match="family='gaussian'"):
        sa.cv_sgdnet(x, cls3, family="multinomial", nfolds=3, mode="covariance", fold_fits="batched")
    with pytest.raises(ValueError, match="more than two classes"):
        sa.cv_newton_fits(x, cls3, fold, 0.5, [0.1, 0.01])
    with pytest.raises(ValueError, match="more than two classes"):
        sa.cv_sgdnet_newton(x, cls3, nfolds=3, nlambda=3)
    assert sa.sgdnet(x, cls3, family="multinomial", nlambda=3, mode="auto").draws_used > 0
    rng_state = sa.RRng(2)
    cv = sa.cv_sgdnet(x, cls3, family="multinomial", nfolds=3, nlambda=3, mode="auto", rng=rng_state, foldid=fold + 1)
    assert cv.fit.draws_used > 0 and bytes(rng_state.state) != bytes(sa.RRng(2).state)
    fits = sa.cv_newton_fits(x, cls2, fold, 0.5, [0.1, 0.01])
    assert len(fits) == 3 and all(f.family == "binomial" and f.beta.shape == (4, 2) for f in fits)
    # ... while the multinomial Newton CV leaves a generator it does not need for fold ids alone
    rng_state = sa.RRng(2)
    cv = sa.cv_sgdnet_mnewton(x, cls3, nfolds=3, nlambda=3, rng=rng_state, foldid=fold + 1, fold_fits="batched")
    assert cv.fit.draws_used == 0 and bytes(rng_state.state) == bytes(sa.RRng(2).state)
