"""sa.cv_wmnewton_fits (sgdnet_amd/csrc/mnewton.hip: wmnewton_cv_run) under both settings of "cv_wmnewton_moments": 0, the tile
kernel on a single wide fit's row chunks, and 1, mnewton_cv_mfma.hip (6 (mix, class pair) members of a training set per workgroup).
A fold fit is BY DEFINITION sa.sgdnet_wmnewton on x[T], y[T].  KKT_BOUND and SAME_OPTIMUM are tests/test_gpu_cv_mnewton.py's; at
mix = 1 and an even K the coefficients are not unique and dev_ratio is compared.  HESSIAN_BOUND is ten times option 0's largest
distance from the float64 restatement of two Newton steps (profiles/cv_wmnewton.txt, section 2)."""
import numpy as np
import pytest
import scipy.sparse as sp

import cv_mnewton_reference as ref
import cv_wnewton_reference as cwr
import test_cv_wmnewton_host as host
import test_gpu_cv_covariance as tcv
import test_gpu_cv_mnewton as tcm
import test_gpu_mnewton as tm
import wmnewton_reference as wr

pytestmark = pytest.mark.gpu

OPTION = "cv_wmnewton_moments"
THRESH = wr.THRESH
OPTION0_FROM_RESTATEMENT = 1.25e-14       # the largest over host.TWO_STEP_EDGES, at (450, 63, 3, 3, 2, "rest") job 0 (profiles/cv_wmnewton.txt, section 2)
HESSIAN_BOUND = 10 * OPTION0_FROM_RESTATEMENT
sa = tcm.sa


def run(sa, setting, *args, **kw):
    with sa.option(OPTION, setting):
        return sa.cv_wmnewton_fits(*args, **kw)


def same_bytes(f, g, what):
    assert tm.stacked(f).tobytes() == tm.stacked(g).tobytes(), (what, "beta")
    for name in ("a0", "dev_ratio", "return_codes"):
        assert getattr(f, name).tobytes() == getattr(g, name).tobytes(), (what, name)
    assert f.npasses == g.npasses > 0 and f.diagnostics == g.diagnostics and f.diagnostics["steps"] > 0 and f.nulldev == g.nulldev, what


def check_every_job(sa, x, y, K, foldid, mixes, lam, train_on, separate=True, **kw):
    """both options: return codes 0 and KKT on x[T], y[T]; option 0 is the separate fit, option 1 the option-0 fit"""
    new, old = (run(sa, s, x, y, foldid, mixes, lam, train_on=train_on, **kw) for s in (1, 0))
    sets = tcv.training_sets(foldid, train_on)
    assert len(new) == len(old) == len(mixes) * len(sets)
    for job, (f, g) in enumerate(zip(new, old)):
        T, mix = sets[job % len(sets)], mixes[job // len(sets)]
        unique = ref.coefficients_are_unique(mix, K)
        for name, fit in (("option 1", f), ("option 0", g)):
            what = (x.shape, K, train_on, len(mixes), job, name)
            assert (fit.return_codes == 0).all() and len(fit.lambda_) == len(lam[0]) and fit.nobs == T.sum(), (what, fit.return_codes)
            assert fit.npasses == 1 + fit.diagnostics["steps"] + fit.diagnostics["halvings"], what
            tm.assert_optimal(sa.kkt(fit, x[T], y[T]), fit.lambda_, what)
        if separate:
            sep = sa.sgdnet_wmnewton(x[T], y[T], alpha=mix, lambda_=lam[job // len(sets)], **kw)
            tcm.assert_same_fit(g, sep, (x.shape, K, train_on, job, "option 0 / separate"), unique)
        tcm.assert_same_fit(f, g, (x.shape, K, train_on, job, "option 1 / option 0"), unique)
    return new


# ---- 1. the edges (host.EDGES: n, p, K, folds, mixes, train_on) ----
# p + 2 = 64, 65, 129 (one, two, three macro tiles); sets of 257 | 256 rows and "rest" sets whose slabs straddle the gap; 3, 9,
# 12, 20 and 6 members: a partial group, a group spanning two mixes, one mix per group, groups that begin in the middle of a mix.

@pytest.mark.parametrize("edge", host.EDGES)
def test_every_job_is_optimal_and_the_separate_fit(sa, edge):
    x, y, foldid = host.edge_input(edge)
    mixes = host.mixes_of(edge[4])
    lam = [host.edge_lambdas(edge, x, y, m) for m in mixes]
    check_every_job(sa, x, y, edge[2], foldid, mixes, lam, edge[5], thresh=THRESH)


# ---- 2. the Hessian itself: the iterate after exactly two Newton steps ----

@pytest.mark.parametrize("edge", host.TWO_STEP_EDGES)
def test_two_newton_steps_are_those_of_option_0(sa, edge):
    x, y, foldid, restated = host.two_step_reference(edge)
    T = host.TWO_STEP
    distance = lambda f, a0, beta: max(np.abs(tm.stacked(f) - beta).max(), np.abs(f.a0 - a0).max()) / np.abs(beta).max()
    kw = dict(train_on=edge[5], standardize=T["standardize"], thresh=T["thresh"], maxit=T["maxit"])
    mixes = [T["mix"]] * 2                                         # (two mixes: 6 members at K = 2, 12 at K = 3)
    new, old = (run(sa, s, x, y, foldid, mixes, [T["lam"]] * 2, **kw) for s in (1, 0))
    for job, (f, g) in enumerate(zip(new, old)):
        a0, beta = restated[job % len(restated)][:2]
        d_ref, d_new = distance(g, a0, beta), distance(f, g.a0, tm.stacked(g))
        print(edge, "job", job, "option 0 from the restatement %.3g, option 1 from option 0 %.3g" % (d_ref, d_new))
        assert f.diagnostics["steps"] == g.diagnostics["steps"] == 2 and f.diagnostics["halvings"] == 0
        assert d_new <= HESSIAN_BOUND, (edge, job, d_new, d_ref)


# ---- 3. independence and determinism, bit for bit: two macro tiles, two chunks ----

@pytest.mark.parametrize("setting", [1, 0])
def test_jobs_are_independent_repeatable_and_the_sparse_call(sa, setting):
    n, p, K, folds = 520, 63, 3, 2                                 # p + 2 = 65; sets of 260 rows: two chunks under option 1
    xs, y = tm.problem(n, p, K, True, seed=6)
    x = np.asarray(xs.todense())
    foldid = ref.equal_folds(n, folds, y, K, seed=6)
    lam = wr.automatic_lambdas(x, y, K, 0.5, True, 4, 0.1)
    mixes = [0.0, 0.5, 1.0]                                        # 18 members: the members of mix 0.5 share groups with both others'
    many = [lam] * 3
    kw = dict(thresh=1e-9)
    alone = run(sa, setting, x, y, foldid, [0.5], [lam], **kw)
    among = run(sa, setting, x, y, foldid, mixes, many, **kw)
    for j in range(folds):
        same_bytes(alone[j], among[folds + j], ("alone / among", setting, j))
    if setting == 0:
        return
    others = dict(again=run(sa, 1, x, y, foldid, mixes, many, **kw), sparse=run(sa, 1, sp.csc_matrix(xs), y, foldid, mixes, many, **kw))
    for width in (256, 1024):
        with sa.option("wmnewton_width", width):
            others["%d lanes" % width] = run(sa, 1, x, y, foldid, mixes, many, **kw)
    for j, f in enumerate(among):
        for name, other in others.items():
            same_bytes(f, other[j], (name, j))


# ---- 4. members of one group at different actions in one round ----

def test_members_of_a_group_at_different_actions(sa):
    """cv_wnewton_reference's halving input as a problem of two classes, two mixes: their 6 members share one group, and in some
    rounds one steps while another halves or has finished.  (No separate fit: at 1e-6 on such data a last-place difference
    moves the whole trajectory.)"""
    x, y, foldid = cwr.halving_input()
    H = cwr.HALVING
    mixes = [H["mix"], 0.9]
    fits = check_every_job(sa, x, y, 2, foldid, mixes, [H["lam"]] * 2, "rest", separate=False, thresh=THRESH, maxit=H["maxit"])
    steps = [f.diagnostics["steps"] for f in fits]
    halvings = [f.diagnostics["halvings"] for f in fits]
    print("halving input, two mixes: steps per job", steps, "halvings per job", halvings)
    assert steps[0] != steps[2] and steps[1] != steps[3] and max(halvings) >= 1, (steps, halvings)


# ---- 5. refusals on the device path, by name, nothing launched ----

def test_refusals_on_the_device_path(sa):
    rng = np.random.default_rng(0)
    cls, fold = (np.arange(18) // 3 % 3).astype(float), np.arange(18) % 3
    with pytest.raises(sa.SgdnetError, match="cv wmnewton needs no more features than sgdnet_wmnewton_max_features") as e:
        sa.cv_wmnewton_fits(rng.standard_normal((18, sa.wmnewton_max_features(3) + 1)), cls, fold, 0.5, [0.1])
    assert e.value.code == -5
    missing = np.where(cls == 0, 0, 1 + np.arange(18) % 2)          # group 0: the rows of class 0 and nothing else
    with pytest.raises(sa.SgdnetError, match="the training set of group 0 of 3 holds no row of class 1") as e:
        sa.cv_wmnewton_fits(rng.standard_normal((18, 4)), cls, missing, 0.5, [0.1])
    assert e.value.code == -1


# ---- 6. option 0 is untouched by a call at option 1 ----

def test_option_0_is_untouched_by_a_call_at_option_1(sa):
    edge = host.EDGES[0]
    x, y, foldid = host.edge_input(edge, seed=6)
    lam = [host.edge_lambdas(edge, x, y, 0.5)]
    before = run(sa, 0, x, y, foldid, [0.5], lam, thresh=1e-9)
    run(sa, 1, x, y, foldid, [0.5], lam, thresh=1e-9)
    after = run(sa, 0, x, y, foldid, [0.5], lam, thresh=1e-9)
    for j, (f, g) in enumerate(zip(before, after)):
        same_bytes(f, g, ("option 0 before / after", j))
