"""Cross-validation in wide Newton mode: every fold fit of every alpha from ONE native call whose jobs advance in lock-step
around the wide inner solve (sa.cv_wnewton_fits -> sgdnet_cv_wnewton_*, sgdnet_amd/csrc/newton.hip: wnewton_cv_run) and
sa.cv_sgdnet_wnewton on top of it.

Fold fit (alpha, fold j) is BY DEFINITION sa.sgdnet_wnewton(x[T], y[T], alpha=alpha, lambda_=lambda) for the training set T of
fold j.  The primary check is independent of any solver: the optimality conditions of that problem on x[T], y[T] (sa.kkt)
within the project's bound, for every job and every lambda.  The second check is the separate fit itself, to the project's
figure for "the same optimum reached twice".

Tolerances (cv_wnewton_reference)
  KKT_BOUND = 1e-8          KKT residual <= 1e-8 * lambda, coefficients and intercept.  tests/test_cv_wnewton_host.py: the numpy
                            restatement of every job of every shape but the limit meets it.
  SAME_OPTIMUM = 1e-9       relative to max|beta|, as tests/test_gpu_cv_covariance.py::assert_same_fit holds it.  Both fits stop
                            at THRESH = 1e-12; the host file measures what the driver's pooled centres cost against the
                            set's own (<= 1e-13).
  the halving input         the penalised objective within cv_wnewton_reference.HALVING_OBJECTIVE_BOUND of the separate fit's:
                            ten times what the two restatements differ by there.

The shapes and inputs, and why each is there: cv_wnewton_reference."""
import numpy as np
import pytest
import scipy.sparse as sp

import cv_wnewton_reference as cr
import test_gpu_cv_covariance as tcv
import test_gpu_newton as tn
import test_gpu_wnewton as tw
import wnewton_reference as wr

pytestmark = pytest.mark.gpu

KKT_BOUND, SAME_OPTIMUM, THRESH = cr.KKT_BOUND, cr.SAME_OPTIMUM, cr.THRESH
MIXES = cr.MIXES
equal_folds, training_sets, assert_optimal, assert_same_fit = cr.equal_folds, cr.training_sets, tn.assert_optimal, tcv.assert_same_fit


@pytest.fixture(scope="module")
def sa():
    import torch  # noqa: F401
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    return sgdnet_amd


def rows(x, T):
    return sp.csc_matrix(sp.csr_matrix(x)[T]) if sp.issparse(x) else x[T]


def check_jobs(sa, x, y, foldid, mixes, train_on, lam, standardize=True, intercept=True, compare=True):
    """one batched call over `mixes`; KKT on x[T], y[T] for every job and lambda, and the separate fit of every job"""
    opts = dict(standardize=standardize, intercept=intercept, thresh=THRESH)
    fits = sa.cv_wnewton_fits(x, y, foldid, mixes, lam, train_on=train_on, **opts)
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
                ref = sa.sgdnet_wnewton(xT, yT, alpha=m, lambda_=lam[a], **opts)
                assert (ref.return_codes == 0).all(), what
                assert_same_fit(fit, ref, yT.mean(), what)
    return fits


def same_bytes(f, g, what):
    for name in ("beta", "a0", "dev_ratio", "return_codes"):
        assert getattr(f, name).tobytes() == getattr(g, name).tobytes(), (what, name)
    assert f.npasses == g.npasses > 0 and f.diagnostics["steps"] == g.diagnostics["steps"] > 0 and f.nulldev == g.nulldev, what
    assert f.diagnostics["halvings"] == g.diagnostics["halvings"], what


# ---- 1. the envelope ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", cr.SHAPES)
def test_every_fold_fit_is_optimal_and_the_separate_fit(sa, shape, sparse, train_on):
    n, p, G = shape[0], cr.features(shape), shape[2]
    assert wr.LIMIT == sa.wnewton_max_features()
    x, y = tn.problem(n, p, sparse)
    mixes = MIXES if shape[1] is not None else [cr.limit_mix(sparse, train_on)]       # (the limit: one mix per case, KKT only)
    lam = [cr.lambdas_of(x, y, shape, m) for m in mixes]
    check_jobs(sa, x, y, equal_folds(n, G), mixes, train_on, lam, compare=shape[1] is not None and p <= cr.COMPARE_UP_TO)


# ---- 2. intercept x standardize ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", [cr.SHAPES[0], cr.SHAPES[2]])
def test_intercept_and_standardize_combinations(sa, shape, sparse, train_on):
    n, p, G = shape
    x, y = tn.problem(n, p, sparse, seed=1)
    for intercept, standardize in ((True, False), (False, True), (False, False)):     # (True, True) is the test above
        lam = [cr.lambdas_of(x, y, shape, m, standardize) for m in MIXES]
        check_jobs(sa, x, y, equal_folds(n, G, seed=1), MIXES, train_on, lam, standardize=standardize, intercept=intercept)


# ---- 3. row chunks: a job of two beside a job of one; a chunk across the gap between a job's two row ranges ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("name", ["two", "gap"])
def test_jobs_of_different_row_chunk_counts(sa, name, train_on):
    x, y, foldid, sizes = cr.row_chunk_inputs()[name]
    chunks = [cr.job_chunks(n_t if train_on == "fold" else 500 - n_t, 1) for n_t in sizes]
    assert chunks == {("two", "fold"): [2, 1], ("two", "rest"): [1, 2], ("gap", "fold"): [1, 1, 1], ("gap", "rest"): [2, 2, 2]}[(name, train_on)]
    lam = [cr.lambdas_of(x, y, (500, 1, len(sizes)), m) for m in MIXES]
    check_jobs(sa, x, y, foldid, MIXES, train_on, lam)


# ---- 4. more jobs than compute units ----

def test_leave_one_out_of_270_jobs(sa):
    x, y, foldid = cr.leave_one_out_input()
    lam = [cr.lambdas_of(x, y, (90, 3, 90), m) for m in MIXES]
    fits = check_jobs(sa, x, y, foldid, MIXES, "rest", lam, compare=False)
    assert len(fits) == 270
    # the separate fit of one job in ten, the first and the last among them
    sets = training_sets(foldid, "rest")
    for job in list(range(0, 270, 10)) + [269]:
        a, j = divmod(job, 90)
        ref = sa.sgdnet_wnewton(x[sets[j]], y[sets[j]], alpha=MIXES[a], lambda_=lam[a], thresh=THRESH)
        assert_same_fit(fits[job], ref, y[sets[j]].mean(), ("leave-one-out", job))


# ---- 5. where the narrow CV runs too ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", cr.BOTH_MODES)
def test_same_optimum_as_the_narrow_cross_validation(sa, shape, sparse, train_on):
    n, p, G = shape
    x, y = tn.problem(n, p, sparse, seed=3)
    mixes = [0.5, 0.0]
    lam = [tn.automatic_lambdas(x, y, m, True, wr.BOTH_MODES_PATH["nlambda"], wr.BOTH_MODES_PATH["lambda_min_ratio"]) for m in mixes]
    foldid = equal_folds(n, G, seed=3)
    wide = sa.cv_wnewton_fits(x, y, foldid, mixes, lam, train_on=train_on, thresh=THRESH)
    narrow = sa.cv_newton_fits(x, y, foldid, mixes, lam, train_on=train_on, thresh=THRESH)
    assert len(wide) == len(narrow) == len(mixes) * G
    for job, (w, nw) in enumerate(zip(wide, narrow)):
        what = (shape, sparse, train_on, job)
        assert (w.return_codes == 0).all() and (nw.return_codes == 0).all(), what
        scale = np.abs(nw.beta).max()
        err = max(np.abs(w.beta - nw.beta).max(), np.abs(w.a0 - nw.a0).max()) / scale
        dev = np.abs(w.dev_ratio - nw.dev_ratio).max()
        print(what, "wide vs narrow CV: coefficients %.3g of max|beta|, dev_ratio %.3g" % (err, dev))
        assert err <= tw.SAME_OPTIMUM_REL and dev <= tw.SAME_DEV_RATIO, (what, err, dev)
        assert w.lambda_.tobytes() == nw.lambda_.tobytes() and w.nobs == nw.nobs
        if not sparse:
            assert w.nulldev == nw.nulldev, what
        else:
            assert abs(w.nulldev - nw.nulldev) <= SAME_OPTIMUM * nw.nulldev, what


# ---- 6. independence and determinism ----

@pytest.mark.parametrize("shape", [(130, 513, 2), (195, 15, 3)])
def test_jobs_are_independent_and_repeatable_at_both_widths(sa, shape):
    n, p, G = shape
    x, y = tn.problem(n, p, False, seed=6)
    foldid = equal_folds(n, G, seed=6)
    lam = cr.lambdas_of(x, y, shape, 0.5)
    kw = dict(thresh=1e-9)
    alone = sa.cv_wnewton_fits(x, y, foldid, [0.5], [lam], **kw)
    among = sa.cv_wnewton_fits(x, y, foldid, [0.2, 0.5, 1.0], [lam, lam, lam], **kw)
    again = sa.cv_wnewton_fits(x, y, foldid, [0.2, 0.5, 1.0], [lam, lam, lam], **kw)
    for j in range(G):
        same_bytes(alone[j], among[G + j], ("alone / among", j))
    for j, (f, g) in enumerate(zip(among, again)):
        same_bytes(f, g, ("again", j))
    with sa.option("wnewton_width", 256):
        narrow = sa.cv_wnewton_fits(x, y, foldid, [0.2, 0.5, 1.0], [lam, lam, lam], **kw)
    with sa.option("wnewton_width", 1024):
        full = sa.cv_wnewton_fits(x, y, foldid, [0.2, 0.5, 1.0], [lam, lam, lam], **kw)
    for j, (f, g, h) in enumerate(zip(narrow, full, among)):
        same_bytes(f, g, ("256 / 1024 lanes", j))
        same_bytes(f, h, ("256 lanes / the rule", j))
    with sa.option("wnewton_width", 512):                      # not a width the library has
        with pytest.raises(sa.SgdnetError) as e:
            sa.cv_wnewton_fits(x, y, foldid, [0.5], [lam], **kw)
    assert e.value.code == -1


# ---- 7. sparse x is the dense call on the same matrix ----

@pytest.mark.parametrize("shape", [(195, 15, 3), (600, 199, 3)])
def test_sparse_call_is_the_dense_call(sa, shape):
    n, p, G = shape
    x, y = tn.problem(n, p, True)
    foldid = equal_folds(n, G)
    lam = [cr.lambdas_of(x, y, shape, m) for m in (0.5, 1.0)]
    for train_on in ("fold", "rest"):
        s = sa.cv_wnewton_fits(x, y, foldid, [0.5, 1.0], lam, train_on=train_on, thresh=THRESH)
        d = sa.cv_wnewton_fits(np.asarray(x.todense()), y, foldid, [0.5, 1.0], lam, train_on=train_on, thresh=THRESH)
        for j, (f, g) in enumerate(zip(s, d)):
            same_bytes(f, g, (shape, train_on, j))


# ---- 8. halved steps, and jobs at different lambdas in one round ----

def test_halved_steps_and_jobs_at_their_own_pace(sa):
    x, y, foldid = cr.halving_input()
    H = cr.HALVING
    kw = dict(thresh=H["thresh"], maxit=H["maxit"])
    fits = sa.cv_wnewton_fits(x, y, foldid, [H["mix"]], [H["lam"]], train_on="rest", **kw)
    sets = training_sets(foldid, "rest")
    assert len(fits) == len(sets) == 2
    steps = [f.diagnostics["steps"] for f in fits]
    halvings = [f.diagnostics["halvings"] for f in fits]
    print("halving input: steps per job", steps, "halvings per job", halvings)
    worst = 0.0
    for j, (fit, T) in enumerate(zip(fits, sets)):
        assert (fit.return_codes == 0).all() and fit.npasses == 1 + steps[j] + halvings[j], (j, fit.return_codes)
        ref = sa.sgdnet_wnewton(x[T], y[T], alpha=H["mix"], lambda_=H["lam"], **kw)
        assert (ref.return_codes == 0).all()
        f_job = cr.objective(fit.a0, fit.beta, x[T], y[T], H["lam"], H["mix"])
        f_ref = cr.objective(ref.a0, ref.beta, x[T], y[T], H["lam"], H["mix"])
        err = (np.abs(f_job - f_ref) / np.abs(f_ref)).max()
        worst = max(worst, err)
        print("job %d: objective against the separate fit's, relative %.3g (separate: npasses %g)" % (j, err, ref.npasses))
    # the halve branch ran, and jobs stood at different lambdas in one round
    assert max(halvings) >= 1 and steps[0] != steps[1], (steps, halvings)
    assert worst <= cr.HALVING_OBJECTIVE_BOUND, worst


# ---- 9. cv_sgdnet_wnewton ----

CV_PATH = dict(nlambda=6, lambda_min_ratio=1e-2)


@pytest.mark.parametrize("train_on", ["fold", "rest"])
def test_cv_sgdnet_wnewton_batched_is_the_separate_cv(sa, train_on):
    x, y = tn.problem(600, 199, False)
    kw = dict(alpha=[0.5, 1], nfolds=3, seed=1, train_on=train_on, thresh=THRESH, **CV_PATH)
    sep = sa.cv_sgdnet_wnewton(x, y, fold_fits="separate", **kw)
    bat = sa.cv_sgdnet_wnewton(x, y, fold_fits="batched", **kw)
    assert np.array_equal(sep.foldid, bat.foldid) and sep.name == bat.name == "Binomial Deviance"
    assert sep.cv_summary.shape == bat.cv_summary.shape and np.array_equal(sep.cv_summary[:, :2], bat.cv_summary[:, :2])
    for a, b in zip(sep.lambda_, bat.lambda_):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(sep.cv_raw, bat.cv_raw):
        err = np.abs(a - b).max() / np.abs(a).max()
        print("600 x 199 %s: cv_raw batched vs separate, relative %.3g" % (train_on, err))
        assert err <= SAME_OPTIMUM
    assert (sep.alpha_min, sep.lambda_min, sep.lambda_1se) == (bat.alpha_min, bat.lambda_min, bat.lambda_1se)
    ref = sa.sgdnet_wnewton(x, y, alpha=bat.fit.alpha, thresh=THRESH, **CV_PATH)
    for fit in (sep.fit, bat.fit):
        assert fit.beta.tobytes() == ref.beta.tobytes() and fit.a0.tobytes() == ref.a0.tobytes() and fit.draws_used == 0


@pytest.mark.parametrize("type_measure", ["deviance", "auc"])
def test_generator_ends_in_the_same_state(sa, type_measure):
    """the fold ids move the generator (and the tie-breaking draws of "auc" do), the fits do not"""
    x, y = tn.problem(600, 199, False)
    state, folds = [], []
    for fold_fits in ("separate", "batched"):
        rng = sa.RRng(3)
        cv = sa.cv_sgdnet_wnewton(x, y, alpha=[0.5, 1.0], nfolds=3, rng=rng, nlambda=3, lambda_min_ratio=0.1, type_measure=type_measure,
                                  fold_fits=fold_fits, train_on="rest")
        state.append(bytes(rng.state))
        folds.append(cv.foldid)
        assert cv.fit.draws_used == 0
    assert state[0] == state[1] and state[0] != bytes(sa.RRng(3).state)       # (sample() for the fold ids moved it)
    assert np.array_equal(folds[0], folds[1])
    if type_measure == "auc":                                                  # ... and so did the tie-breaking draws, beyond sample()
        rng = sa.RRng(3)
        rng.sample(x.shape[0])
        assert state[0] != bytes(rng.state)
    else:                                                                      # deviance: sample() alone
        rng = sa.RRng(3)
        rng.sample(x.shape[0])
        assert state[0] == bytes(rng.state)
    # with fold ids given, a generator the CV does not need comes back as it went
    rng = sa.RRng(2)
    cv = sa.cv_sgdnet_wnewton(x, y, nfolds=3, nlambda=3, lambda_min_ratio=0.1, rng=rng, foldid=np.arange(600) % 3 + 1, fold_fits="batched")
    assert cv.fit.draws_used == 0 and bytes(rng.state) == bytes(sa.RRng(2).state)
