"""Cross-validation in Newton mode: every fold fit of every alpha from ONE native call whose jobs advance in lock-step
(sa.cv_newton_fits -> sgdnet_cv_newton_*, sgdnet_amd/csrc/newton.hip: newton_cv_run) and sa.cv_sgdnet_newton on top of it.

Fold fit (alpha, fold j) is BY DEFINITION sa.sgdnet_newton(x[T], y[T], alpha=alpha, lambda_=lambda) for the training set T
of fold j.  The primary check is independent of any solver: the optimality conditions of that problem on x[T], y[T] (sa.kkt)
within the project's bound, for every job and every lambda.  The second check is the separate fit itself, to the project's
figure for "the same optimum reached twice".

Tolerances
  KKT_BOUND = 1e-8          KKT residual <= 1e-8 * lambda, coefficients and intercept: tests/test_gpu_covariance.py.
  SAME_OPTIMUM = 1e-9       relative to max|beta|; a0 and dev_ratio as tests/test_gpu_cv_covariance.py::assert_same_fit holds
                            them.  Both fits stop at thresh = 1e-12; tests/test_cv_newton_host.py measures what a different
                            centre of the Newton problem costs at that thresh (<= 1e-10).

The shapes (n, p, folds): groups of 64 and 65 rows straddle the 64-row stage of the moments pass; p + 2 = 16, 17 and 18
straddle its 16-column tile; ten uneven groups give 30 jobs over several state-pass workgroups; the last shape sits at the
limit of one workgroup's LDS.  The lambdas are the driver's automatic path of the whole data (tn.automatic_lambdas), handed
to every job as user lambdas."""
import numpy as np
import pytest
import scipy.sparse as sp

import test_gpu_cv_covariance as tcv
import test_gpu_newton as tn

pytestmark = pytest.mark.gpu

KKT_BOUND = tn.KKT_BOUND
SAME_OPTIMUM = tcv.SAME_OPTIMUM
SHAPES = [(37, 2, 3), (192, 14, 3), (195, 15, 3), (195, 16, 3), (1003, 33, 10), (1800, None, 3)]     # None: newton_max_features()
NLAMBDA, THRESH = 8, tn.THRESH
MIXES = [0.0, 0.5, 1.0]

equal_folds, training_sets, assert_optimal, assert_same_fit = tcv.equal_folds, tcv.training_sets, tn.assert_optimal, tcv.assert_same_fit


@pytest.fixture(scope="module")
def sa():
    import torch  # noqa: F401
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    return sgdnet_amd


def rows(x, T):
    return sp.csc_matrix(sp.csr_matrix(x)[T]) if sp.issparse(x) else x[T]


def check_jobs(sa, x, y, foldid, mixes, train_on, standardize=True, intercept=True, compare=True, nlambda=NLAMBDA, lambda_min_ratio=1e-2,
               lam=None):
    """one batched call over `mixes`; KKT on x[T], y[T] for every job and lambda, and the separate fit of every job"""
    opts = dict(standardize=standardize, intercept=intercept, thresh=THRESH)
    if lam is None:
        lam = [tn.automatic_lambdas(x, y, m, standardize, nlambda, lambda_min_ratio) for m in mixes]
    fits = sa.cv_newton_fits(x, y, foldid, mixes, lam, train_on=train_on, **opts)
    sets = training_sets(foldid, train_on)
    assert len(fits) == len(mixes) * len(sets)
    for a, m in enumerate(mixes):
        for j, T in enumerate(sets):
            fit, xT, yT = fits[a * len(sets) + j], rows(x, T), y[T]
            what = (x.shape, sp.issparse(x), m, train_on, standardize, intercept, j)
            assert (fit.return_codes == 0).all() and fit.draws_used == 0 and fit.alpha == m and fit.family == "binomial", what
            assert np.array_equal(fit.lambda_, lam[a]) and np.isfinite(fit.dev_ratio).all() and fit.nobs == T.sum()
            assert fit.npasses == 1 + fit.diagnostics["steps"] + fit.diagnostics["halvings"] and fit.diagnostics["steps"] >= len(lam[a])
            assert_optimal(sa.kkt(fit, xT, yT, standardize=standardize, intercept=intercept), fit.lambda_, what)     # no job, no lambda dropped
            if compare:
                ref = sa.sgdnet_newton(xT, yT, alpha=m, lambda_=lam[a], **opts)
                assert_same_fit(fit, ref, yT.mean(), what)
    return fits


# ---- 1. the envelope ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_fold_fit_is_optimal_and_the_separate_fit(sa, shape, sparse, train_on):
    n, p, G = shape[0], shape[1] or tn.pmax(), shape[2]
    x, y = tn.problem(n, p, sparse)
    if shape[1] is None:
        # at the largest p one mix per case, rotated so that the four cases of this shape see all three; KKT only
        mix = MIXES[(2 * sparse + (train_on == "rest") + 1) % 3]
        check_jobs(sa, x, y, equal_folds(n, G), [mix], train_on, compare=False, lambda_min_ratio=tn.ratio_for(p))
    else:
        check_jobs(sa, x, y, equal_folds(n, G), MIXES, train_on)


# ---- 2. intercept x standardize ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]])
def test_intercept_and_standardize_combinations(sa, shape, sparse, train_on):
    n, p, G = shape
    x, y = tn.problem(n, p, sparse, seed=1)
    for intercept, standardize in ((True, False), (False, True), (False, False)):     # (True, True) is the test above
        check_jobs(sa, x, y, equal_folds(n, G, seed=1), MIXES, train_on, standardize=standardize, intercept=intercept)


# ---- 3. awkward folds ----

@pytest.mark.parametrize("sparse", [False, True])
def test_folds_cut_along_a_sorted_column(sa, sparse):
    """every fold's mean of column 0 sits far from the whole-data mean the per-group sums are taken about"""
    n, p, G = 195, 15, 3
    x, y = tn.problem(n, p, sparse, seed=2)
    col = np.asarray(x[:, 0].todense()).ravel() if sparse else x[:, 0]
    foldid = np.empty(n, dtype=np.int64)
    foldid[np.argsort(col, kind="stable")] = np.arange(n) * G // n
    for train_on in ("fold", "rest"):
        check_jobs(sa, x, y, foldid, [0.5, 1.0], train_on)


@pytest.mark.parametrize("sparse", [False, True])
def test_unequal_groups_with_arbitrary_labels(sa, sparse):
    n, p = 150, 5
    x, y = tn.problem(n, p, sparse, seed=3)
    foldid = np.repeat([10, 20, 30, 40], [3, 47, 65, 35])          # labels need not be 1..G; a group of three rows
    foldid = foldid[np.random.default_rng(3).permutation(n)]
    check_jobs(sa, x, y, foldid, [0.5, 1.0], "rest")
    keep = foldid != 10                                             # (three rows cannot hold two of each class and five features)
    check_jobs(sa, rows(x, keep), y[keep], foldid[keep], [0.5, 1.0], "fold")


@pytest.mark.parametrize("sparse", [False, True])
def test_leave_one_out(sa, sparse):
    n, p = 12, 2
    x, y = tn.problem(n, p, sparse, seed=4)
    check_jobs(sa, x, y, np.arange(n), [0.5, 1.0], "rest")          # nfolds = n


@pytest.mark.parametrize("sparse", [False, True])
def test_large_mean_column(sa, sparse):
    """a column of mean 1e6 and sd 1 (every entry stored): KKT on x[T], y[T] only, on the path of
    tests/test_gpu_cv_covariance.py::test_large_mean_column (lambda_min_ratio = 0.05) for the reason given there: a0 is of the
    order of 1e6 times the column's coefficient, and KKT_BOUND * lambda has to stay above one unit in its last place."""
    n, p, G = 195, 5, 3
    x, _ = tn.problem(n, p, sparse, seed=5)
    xd = np.asarray(x.todense()) if sparse else x.copy()
    rng = np.random.default_rng(11)
    col = rng.standard_normal(n)
    col = (col - col.mean()) / col.std()
    eta = 0.4 * (xd[:, 0] - xd[:, 0].mean()) + 0.7 * col
    xd[:, 2] = 1e6 + col
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
    x = sp.csc_matrix(xd) if sparse else xd
    for train_on in ("fold", "rest"):
        check_jobs(sa, x, y, equal_folds(n, G, seed=5), [0.5, 1.0], train_on, compare=False, nlambda=10, lambda_min_ratio=0.05)


# ---- 4. jobs at different lambdas in one round ----

def steep_problem(sparse):
    """n = 195, p = 5 and a steep logistic signal: the Newton steps from lambda to lambda are long, and some are halved"""
    n, p = 195, 5
    rng = np.random.default_rng(42)
    x = rng.standard_normal((n, p)) * rng.uniform(0.5, 3.0, p) + rng.uniform(-2.0, 2.0, p)
    if sparse:
        keep = rng.random((n, p)) < 0.5
        keep[0, :] = True
        x = x * keep
    z = (x - x.mean(axis=0)) / x.std(axis=0)
    eta = 4.0 * z[:, 0] - 3.0 * z[:, 1] + 0.5
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
    return (sp.csc_matrix(x) if sparse else x), y


STEEP_LAMBDAS = [2e-3, 5e-2, 5e-4]


@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
def test_jobs_progress_at_their_own_pace(sa, sparse, train_on):
    x, y = steep_problem(sparse)
    mixes = [0.5, 1.0]
    fits = check_jobs(sa, x, y, equal_folds(195, 3, seed=6), mixes, train_on, compare=False, lam=[np.array(STEEP_LAMBDAS)] * 2)
    steps = [f.diagnostics["steps"] for f in fits]
    print("steps per job", steps, "halvings per job", [f.diagnostics["halvings"] for f in fits])
    # the jobs need different numbers of steps: the lock-step loop ran jobs at different lambdas in the same round
    assert len(set(steps)) > 1, steps


# ---- 5. independence and determinism ----

@pytest.mark.parametrize("sparse", [False, True])
def test_jobs_are_independent_and_repeatable(sa, sparse):
    n, p, G = 1003, 33, 10
    x, y = tn.problem(n, p, sparse, seed=6)
    foldid = equal_folds(n, G, seed=6)
    lam = np.geomspace(0.1, 0.002, 6)
    kw = dict(thresh=1e-9)
    alone = sa.cv_newton_fits(x, y, foldid, [0.5], [lam], **kw)
    among = sa.cv_newton_fits(x, y, foldid, [0.2, 0.5, 1.0], [lam, lam, lam], **kw)
    again = sa.cv_newton_fits(x, y, foldid, [0.2, 0.5, 1.0], [lam, lam, lam], **kw)

    def same(f, g, what):
        for name in ("beta", "a0", "dev_ratio", "return_codes"):
            assert getattr(f, name).tobytes() == getattr(g, name).tobytes(), (what, name)
        assert f.npasses == g.npasses > 0 and f.diagnostics["steps"] == g.diagnostics["steps"] > 0 and f.nulldev == g.nulldev, what

    for j in range(G):
        same(alone[j], among[G + j], ("alone / among", j))
    for j, (f, g) in enumerate(zip(among, again)):
        same(f, g, ("again", j))


# ---- 6. cv_sgdnet_newton on abalone ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
def test_cv_sgdnet_newton_batched_is_the_separate_cv_on_abalone(sa, train_on):
    x, y = tn.abalone_binomial()
    kw = dict(alpha=[0.5, 1], nfolds=5, seed=1, train_on=train_on, thresh=THRESH, nlambda=20)
    sep = sa.cv_sgdnet_newton(x, y, fold_fits="separate", **kw)
    bat = sa.cv_sgdnet_newton(x, y, fold_fits="batched", **kw)
    assert np.array_equal(sep.foldid, bat.foldid) and sep.name == bat.name == "Binomial Deviance"
    assert sep.cv_summary.shape == bat.cv_summary.shape and np.array_equal(sep.cv_summary[:, :2], bat.cv_summary[:, :2])
    for a, b in zip(sep.lambda_, bat.lambda_):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(sep.cv_raw, bat.cv_raw):
        err = np.abs(a - b).max() / np.abs(a).max()
        print("abalone %s: cv_raw batched vs separate, relative %.3g" % (train_on, err))
        assert err <= SAME_OPTIMUM
    assert (sep.alpha_min, sep.lambda_min, sep.lambda_1se) == (bat.alpha_min, bat.lambda_min, bat.lambda_1se)
    ref = sa.sgdnet_newton(x, y, alpha=bat.fit.alpha, nlambda=20, thresh=THRESH)
    for fit in (sep.fit, bat.fit):
        assert fit.beta.tobytes() == ref.beta.tobytes() and fit.a0.tobytes() == ref.a0.tobytes() and fit.draws_used == 0


@pytest.mark.parametrize("type_measure", ["deviance", "auc"])
def test_generator_ends_in_the_same_state(sa, type_measure):
    x, y = tn.abalone_binomial()
    state, folds = [], []
    for fold_fits in ("separate", "batched"):
        rng = sa.RRng(3)
        cv = sa.cv_sgdnet_newton(x, y, alpha=[0.5, 1.0], nfolds=3, rng=rng, nlambda=5, type_measure=type_measure, fold_fits=fold_fits)
        state.append(bytes(rng.state))
        folds.append(cv.foldid)
    assert state[0] == state[1] and state[0] != bytes(sa.RRng(3).state)       # (sample() for the fold ids moved it)
    assert np.array_equal(folds[0], folds[1])
    if type_measure == "auc":                                                  # ... and so did the tie-breaking draws, beyond sample()
        rng = sa.RRng(3)
        rng.sample(x.shape[0])
        assert state[0] != bytes(rng.state)


# ---- 7. refusals ----

def test_refusals_name_the_condition(sa):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    score = x[:, 0] + rng.standard_normal(60)
    cls = (score > 0).astype(float)
    fold = np.arange(60) % 3
    pm = sa.newton_max_features()

    def refused(code, needle, xx, yy, ff, alpha=0.5, **kw):
        with pytest.raises(sa.SgdnetError) as e:
            sa.cv_newton_fits(xx, yy, ff, alpha, [[0.1, 0.01]] * np.size(alpha) if np.ndim(alpha) else [0.1, 0.01], **kw)
        assert e.value.code == code and needle in str(e.value), str(e.value)

    wide = rng.standard_normal((30, pm + 1))
    wide_cls = (wide[:, 0] > 0).astype(float)
    refused(-5, "mode = newton needs no more features than sgdnet_newton_max_features()", wide, wide_cls, np.arange(30) % 3)
    refused(-5, "mode = newton needs no more features", sp.csc_matrix(wide), wide_cls, np.arange(30) % 3)
    big = rng.standard_normal((300, pm))
    refused(-5, "mode = newton needs the jobs' workspace within", big, (big[:, 0] > 0).astype(float), np.arange(300), alpha=list(np.linspace(0, 1, 8)),
            train_on="rest")
    one_class = fold.copy()
    one_class[np.argsort(cls, kind="stable")[:20]] = 0              # group 0: twenty rows of class 0 and nothing else
    one_class[np.argsort(cls, kind="stable")[20:]] = 1 + np.arange(40) % 2
    refused(-1, "training set of group 0 of 3 holds one class only", x, cls, one_class)
    with pytest.raises(ValueError, match="more than two classes"):
        sa.cv_newton_fits(x, np.digitize(score, [-0.5, 0.5]), fold, 0.5, [0.1, 0.01])
    # sgdnet() and cv_sgdnet() are as they were: sgdnet() does not know the mode, batched fold fits are covariance mode's,
    # and the SAGA modes still draw
    with pytest.raises(ValueError, match="mode must be one of 'exact', 'batched', 'auto', 'covariance'$"):
        sa.sgdnet(x, cls, family="binomial", nlambda=3, mode="newton")
    with pytest.raises(ValueError, match="mode must be one of"):
        sa.cv_sgdnet(x, cls, family="binomial", nfolds=3, nlambda=3, mode="newton")
    with pytest.raises(ValueError, match="family='gaussian'"):
        sa.cv_sgdnet(x, cls, family="binomial", nfolds=3, mode="covariance", fold_fits="batched")
    assert sa.sgdnet(x, cls, family="binomial", nlambda=3, mode="auto").draws_used > 0
    rng_state = sa.RRng(2)
    cv = sa.cv_sgdnet(x, cls, family="binomial", nfolds=3, nlambda=3, mode="auto", rng=rng_state, foldid=fold + 1)
    assert cv.fit.draws_used > 0 and bytes(rng_state.state) != bytes(sa.RRng(2).state)
    # ... while the Newton CV leaves a generator it does not need for fold ids alone
    rng_state = sa.RRng(2)
    cv = sa.cv_sgdnet_newton(x, cls, nfolds=3, nlambda=3, rng=rng_state, foldid=fold + 1, fold_fits="batched")
    assert cv.fit.draws_used == 0 and bytes(rng_state.state) == bytes(sa.RRng(2).state)
