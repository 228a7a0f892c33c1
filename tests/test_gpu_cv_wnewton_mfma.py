"""The matrix-core moments pass of the wide Newton cross-validation (sgdnet_amd/csrc/newton_cv_mfma.hip, the option
"cv_wnewton_moments" = 1) through sa.cv_wnewton_fits.  A workgroup of it serves a group of G = 6 mixes of one training set on
a pair of 64-column macro tiles over a chunk of at least 256 of the set's rows, 32 rows a slab.

Bounds: KKT_BOUND, SAME_OPTIMUM and THRESH are cv_wnewton_reference's.  HESSIAN_BOUND (the iterate after exactly two Newton
steps, option 1 against option 0, relative to max|beta|) is ten times the largest distance of option 0 from the float64
restatement of those two steps on the same inputs: both are float64 sums in another order, and ten covers the longer chains
of a 64-wide tile.  Source: profiles/cv_wnewton_mfma.txt, section 2."""
import numpy as np
import pytest
import scipy.sparse as sp

import cv_wnewton_reference as cr
import test_cv_wnewton_mfma_host as host
import test_gpu_cv_covariance as tcv
import test_gpu_cv_wnewton as tcw
import test_gpu_newton as tn

pytestmark = pytest.mark.gpu

G = 6                                     # csrc/newton.hpp: kWnewtonCvMfmaGroup
OPTION = "cv_wnewton_moments"
OPTION0_FROM_RESTATEMENT = 9.69e-15       # the largest over host.TWO_STEP_SHAPES, at (385, 127, 3, "rest") (profiles/cv_wnewton_mfma.txt)
HESSIAN_BOUND = 10 * OPTION0_FROM_RESTATEMENT
sa = tcw.sa


def mixes_of(count):
    return [0.5] if count == 1 else list(np.linspace(0.0, 1.0, count))


def run(sa, setting, *args, **kw):
    with sa.option(OPTION, setting):
        return sa.cv_wnewton_fits(*args, **kw)


def check_every_job(sa, x, y, foldid, mixes, lam, train_on, **kw):
    """option 1: every return code 0, KKT on x[T], y[T], and the fit of the option-0 call; no job, no lambda left out"""
    new, old = (run(sa, s, x, y, foldid, mixes, lam, train_on=train_on, **kw) for s in (1, 0))
    sets = cr.training_sets(foldid, train_on)
    assert len(new) == len(old) == len(mixes) * len(sets)
    for job, (f, g) in enumerate(zip(new, old)):
        T = sets[job % len(sets)]
        what = (x.shape, train_on, len(mixes), job)
        assert (f.return_codes == 0).all() and len(f.lambda_) == len(lam[0]) and f.nobs == T.sum(), (what, f.return_codes)
        tn.assert_optimal(sa.kkt(f, x[T], y[T]), f.lambda_, what)
        tcv.assert_same_fit(f, g, y[T].mean(), what)
    return new


# ---- 1. the edges ----
# p + 2 = 64, 65, 129: one macro tile, a second that holds column p + 1 only, three.  Training sets of 257 | 256 rows (two
# chunks, the second of one row, beside one chunk), 300 (the second chunk ends in a slab of 12 rows), 256 | 257 | 257.  "rest"
# with three groups: the held-out group first, in the middle (a slab straddles the gap: 150 and 129 are no multiples of 32)
# and last.  1, G and G + 1 mixes: a group of one, a full group, both.
EDGES = [(513, 62, 2, 1, "fold"), (450, 63, 3, G, "rest"), (385, 127, 3, G + 1, "rest"), (520, 63, 2, G + 1, "fold")]


@pytest.mark.parametrize("n, p, folds, mixes, train_on", EDGES)
def test_every_job_is_optimal_and_the_option_0_fit(sa, n, p, folds, mixes, train_on):
    x, y = tn.problem(n, p, False, seed=1)
    mixes = mixes_of(mixes)
    lam = [cr.lambdas_of(x, y, (n, p, folds), m) for m in mixes]
    check_every_job(sa, x, y, cr.equal_folds(n, folds, seed=1), mixes, lam, train_on, thresh=cr.THRESH)


# ---- 2. the Hessian itself: the iterate after exactly two Newton steps ----

def distance(a0, beta, b0, bb):
    return max(np.abs(beta - bb).max(), np.abs(a0 - b0).max()) / np.abs(bb).max()


@pytest.mark.parametrize("shape", host.TWO_STEP_SHAPES)
def test_two_newton_steps_are_those_of_option_0(sa, shape):
    x, y, foldid, restated = host.two_step_reference(shape)
    T = host.TWO_STEP
    kw = dict(train_on=shape[3], standardize=T["standardize"], thresh=T["thresh"], maxit=T["maxit"])
    mixes = [T["mix"]] * 2                                         # (a group of two members)
    new, old = (run(sa, s, x, y, foldid, mixes, [T["lam"]] * 2, **kw) for s in (1, 0))
    for job, (f, g) in enumerate(zip(new, old)):
        a0, beta, _ = restated[job % len(restated)]
        d_ref, d_new = distance(g.a0, g.beta, a0, beta), distance(f.a0, f.beta, g.a0, g.beta)
        print(shape, "job", job, "option 0 from the restatement %.3g, option 1 from option 0 %.3g" % (d_ref, d_new))
        assert f.diagnostics["steps"] == g.diagnostics["steps"] == 2 and f.diagnostics["halvings"] == 0
        assert d_new <= HESSIAN_BOUND, (shape, job, d_new, d_ref)


# ---- 3. independence and determinism, bit for bit: two macro tiles, two chunks ----

def test_jobs_are_independent_repeatable_and_the_sparse_call(sa):
    n, p, folds = 520, 63, 2
    xs, y = tn.problem(n, p, True, seed=6)
    x = np.asarray(xs.todense())
    foldid = cr.equal_folds(n, folds, seed=6)
    lam = cr.lambdas_of(x, y, (n, p, folds), 0.5)
    mixes = mixes_of(G + 1)
    at = mixes.index(0.5)
    many = [lam] * len(mixes)
    kw = dict(thresh=1e-9)
    alone = run(sa, 1, x, y, foldid, [0.5], [lam], **kw)
    among = run(sa, 1, x, y, foldid, mixes, many, **kw)
    again = run(sa, 1, x, y, foldid, mixes, many, **kw)
    sparse = run(sa, 1, sp.csc_matrix(xs), y, foldid, mixes, many, **kw)
    with sa.option("wnewton_width", 256):
        narrow = run(sa, 1, x, y, foldid, mixes, many, **kw)
    with sa.option("wnewton_width", 1024):
        full = run(sa, 1, x, y, foldid, mixes, many, **kw)
    for j in range(folds):
        tcw.same_bytes(alone[j], among[at * folds + j], ("alone / among", j))
    for j, f in enumerate(among):
        for name, other in (("again", again), ("sparse", sparse), ("256 lanes", narrow), ("1024 lanes", full)):
            tcw.same_bytes(f, other[j], (name, j))


# ---- 4. a group whose members stand at different actions in one round ----

def test_members_of_a_group_at_different_actions(sa):
    """the halving input with the lasso added to its mix: the two members of a set's group take different numbers of steps, so
    in some rounds one steps while the other halves or has finished.  Fitted at THRESH as the cases of 1 are: stopped at
    HALVING's 1e-9 the first lambda's KKT ratio is 3.9e-8 under either setting of the option, which KKT_BOUND does not allow."""
    x, y, foldid = cr.halving_input()
    H = cr.HALVING
    mixes = [H["mix"], 1.0]
    fits = check_every_job(sa, x, y, foldid, mixes, [H["lam"]] * 2, "rest", thresh=cr.THRESH, maxit=H["maxit"])
    steps = [f.diagnostics["steps"] for f in fits]
    halvings = [f.diagnostics["halvings"] for f in fits]
    print("halving input, two mixes: steps per job", steps, "halvings per job", halvings)
    assert steps[0] != steps[2] and steps[1] != steps[3] and max(halvings) >= 1, (steps, halvings)


# ---- 5. option 0 is the parent ----

def test_option_0_is_untouched_by_a_call_at_option_1(sa):
    shape = (195, 15, 3)
    x, y = tn.problem(shape[0], shape[1], False, seed=6)
    foldid = cr.equal_folds(shape[0], shape[2], seed=6)
    lam = [cr.lambdas_of(x, y, shape, 0.5)]
    before = run(sa, 0, x, y, foldid, [0.5], lam, thresh=1e-9)
    run(sa, 1, x, y, foldid, [0.5], lam, thresh=1e-9)
    after = run(sa, 0, x, y, foldid, [0.5], lam, thresh=1e-9)
    for j, (f, g) in enumerate(zip(before, after)):
        tcw.same_bytes(f, g, ("option 0 before / after", j))
