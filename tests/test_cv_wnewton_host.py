"""Cross-validation in wide Newton mode (sgdnet_cv_wnewton_*, sa.cv_wnewton_fits, sa.cv_sgdnet_wnewton), the parts a CPU can
check: the three layers agree on the new names, the Python functions validate their arguments, the native entry points
refuse what they refuse before a device is looked for, and the inputs and the bounds of tests/test_gpu_cv_wnewton.py are sound.

The bounds are the project's own (cv_wnewton_reference): KKT_BOUND, SAME_OPTIMUM, THRESH.  What this file measures for them:
  * the restatement of every job of every shape but the feature limit reaches KKT_BOUND, so the GPU test asks nothing the
    number format does not give;
  * a job solved about the centres and scales the driver pools against the same job about its training set's own: the
    largest difference of coefficients and intercept relative to max|beta| over the shapes up to p = 256 is printed and held
    to SAME_OPTIMUM / 10 (measured 7.2e-14; tests/test_cv_newton_host.py measures <= 1e-10 for the narrow mode, whose centres
    differ more: the whole data's against the set's own);
  * the halving input (see test_the_halving_input_halves_and_its_jobs_differ)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import cv_wnewton_reference as cr
import test_gpu_newton as tn
import wnewton_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_BYTES = 16 << 30                    # newton.hpp: kWnewtonCvBytes


def workspace_bytes(jobs, n, p, n_lambda, max_chunks):
    """newton.hpp: wnewton_cv_bytes, restated"""
    P, ld = p + 1, (p + 1 + 15) // 16 * 16
    per_job = (2 * n + (p + 2) ** 2 + max_chunks * cr.tile_pairs(p + 2) * 256 + ld * P + 2 * P + n_lambda * P + 3 * 1024 + 2 + 8 + 3 * P)
    return 8 * (jobs * per_job + n * p + n)


def test_header_binding_and_package_agree():
    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sgdnet_hip.h")).read()
    assert int(re.search(r"#define SGDNET_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 6       # additions only
    for name in ("sgdnet_cv_wnewton_dense", "sgdnet_cv_wnewton_sparse"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.EXPORTS and hasattr(sa.load(), name), name
    for name in ("cv_wnewton_fits", "cv_sgdnet_wnewton"):
        assert name in sa.__all__ and callable(getattr(sa, name)), name
    # no second layout: the result is sgdnet_cv_newton_result under another name, and the arguments are sgdnet_cv_newton_*'s
    assert re.search(r"typedef sgdnet_cv_newton_result sgdnet_cv_wnewton_result;", hdr)
    assert len(re.findall(r"typedef struct sgdnet_cv_w?newton_result", hdr)) == 1
    narrow = re.search(r"int sgdnet_cv_newton_dense\((.*?)\);", hdr, re.S).group(1)
    wide = re.search(r"int sgdnet_cv_wnewton_dense\((.*?)\);", hdr, re.S).group(1)
    assert " ".join(narrow.split()).replace("sgdnet_cv_newton_result", "sgdnet_cv_wnewton_result") == " ".join(wide.split())
    L = sa.load()
    assert [str(t) for t in L.sgdnet_cv_wnewton_dense.argtypes] == [str(t) for t in L.sgdnet_cv_newton_dense.argtypes]
    assert [str(t) for t in L.sgdnet_cv_wnewton_sparse.argtypes] == [str(t) for t in L.sgdnet_cv_newton_sparse.argtypes]
    # the workspace bound is a named constant whose value the header states, and the worked examples are asserted
    newton_hpp = open(os.path.join(ROOT, "sgdnet_amd", "csrc", "newton.hpp")).read()
    assert re.search(r"kWnewtonCvBytes = \(size_t\)16 << 30;", newton_hpp) and "above 16 GiB" in hdr
    assert "constexpr size_t wnewton_cv_bytes(" in newton_hpp and newton_hpp.count("static_assert(wnewton_cv_bytes(") >= 3
    # ... and they are what the restatement here gives: 50 jobs at p = 1000 and 3000, 25 jobs at the limit and not 26
    assert workspace_bytes(50, 2000, 1000, 100, 1) // 10 ** 7 == 107 and workspace_bytes(50, 2000, 3000, 100, 1) // 10 ** 7 == 921
    assert workspace_bytes(25, 2000, wr.LIMIT, 100, 1) <= BUDGET_BYTES < workspace_bytes(26, 2000, wr.LIMIT, 100, 1)


def test_python_argument_checks():
    import sgdnet_amd as sa
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = (x[:, 0] + rng.standard_normal(60) > 0).astype(float)
    fold = np.arange(60) % 3
    for needle, args, kw in (("one array per alpha", ([0.5, 1.0], [[0.1, 0.01]]), {}),
                             ("must be positive", (0.5, [0.1, -0.01]), {}),
                             ("train_on must be", (0.5, [0.1]), dict(train_on="others")),
                             ("must be in \\[0, 1\\]", (1.5, [0.1]), {}),
                             ("cannot be negative", (0.5, [0.1]), dict(thresh=-1.0)),
                             ("negative or zero", (0.5, [0.1]), dict(maxit=0)),
                             ("must be logical", (0.5, [0.1]), dict(intercept=1))):
        with pytest.raises(ValueError, match=needle):
            sa.cv_wnewton_fits(x, y, fold, *args, **kw)
    with pytest.raises(ValueError, match="must match"):
        sa.cv_wnewton_fits(x, y, fold[:-1], 0.5, [0.1])
    with pytest.raises(ValueError, match="more than two classes"):
        sa.cv_wnewton_fits(x, np.arange(60) % 3, fold, 0.5, [0.1])
    with pytest.raises(ValueError, match="only one class"):
        sa.cv_wnewton_fits(x, np.ones(60), fold, 0.5, [0.1])
    for needle, kw in (("'separate' or 'batched'", dict(fold_fits="fused")), ("train_on must be", dict(train_on="others")),
                       ("nfolds > 2", dict(nfolds=2)), ("'arg' should be one of", dict(type_measure="r2")),
                       ("more folds than samples", dict(nfolds=61)),
                       ("need a list of lambdas", dict(alpha=[0.5, 1.0], lambda_=[0.1, 0.01]))):
        with pytest.raises(ValueError, match=needle):
            sa.cv_sgdnet_wnewton(x, y, **kw)
    with pytest.raises(TypeError):
        sa.cv_sgdnet_wnewton(x, y, mode="auto")                                    # the mode is not an argument: every fit is wide Newton's
    # a valid call reaches the backend: without a device that is where it ends
    if sa.load().sgdnet_device_count() < 1:
        for xx in (x, sp.csc_matrix(x)):
            with pytest.raises(sa.SgdnetError) as e:
                sa.cv_wnewton_fits(xx, y, fold, [0.5, 1.0], [[0.1, 0.01]] * 2, train_on="rest")
            assert e.value.code == -2, str(e.value)
    else:
        assert len(sa.cv_wnewton_fits(x, y, fold, [0.5, 1.0], [[0.1, 0.01]] * 2, train_on="rest")) == 6


def test_native_refusals_name_the_condition():
    """every one of them is decided before any HIP call: they are the same with and without a device"""
    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = (x[:, 0] + rng.standard_normal(60) > 0).astype(float)
    fold = np.arange(60) % 3
    limit = sa.wnewton_max_features()
    assert limit == wr.LIMIT

    def refused(code, needle, xx, yy, ff, alpha=0.5, **kw):
        with pytest.raises(sa.SgdnetError) as e:
            sa.cv_wnewton_fits(xx, yy, ff, alpha, [[0.1, 0.01]] * np.size(alpha) if np.ndim(alpha) else [0.1, 0.01], **kw)
        assert e.value.code == code and needle in str(e.value), str(e.value)

    few = np.arange(12) % 3
    few_cls = (np.arange(12) // 3 % 2).astype(float)                 # every group of four rows holds two of each class
    wide = rng.standard_normal((12, limit + 1))
    refused(-5, "mode = wnewton needs no more features than sgdnet_wnewton_max_features()", wide, few_cls, few)
    refused(-5, "features (limit %d)" % limit, wide, few_cls, few)
    refused(-5, "mode = wnewton needs no more features", sp.csc_matrix(wide), few_cls, few)
    # the dense copy of a sparse x: 70 000 x 2000 x 8 bytes is more than 1 GiB; nothing is stored, so nothing that large is made
    tall = sp.csc_matrix((70_000, 2000))
    tall_cls = (np.arange(70_000) % 2).astype(float)
    refused(-5, "mode = wnewton needs the dense copy of a sparse x", tall, tall_cls, np.arange(70_000) // 2 % 3)
    refused(-5, "70000 samples, 2000 features", tall, tall_cls, np.arange(70_000) // 2 % 3)
    # the workspace: at the feature limit a job is 0.68 GB whatever its rows; 8 mixes x 3 folds are 24 jobs and fit the 16 GiB
    # (the arithmetic of newton.hpp, restated above), 9 x 3 = 27 do not
    assert workspace_bytes(24, 12, limit, 2, 1) <= BUDGET_BYTES < workspace_bytes(27, 12, limit, 2, 1)
    at_limit = wide[:, :limit]
    refused(-5, "mode = wnewton needs the jobs' workspace within %d bytes: 9 mixes x 3 groups of 12 rows and %d features" % (BUDGET_BYTES, limit),
            at_limit, few_cls, few, alpha=list(np.linspace(0, 1, 9)))
    refused(-5, "are %d bytes" % workspace_bytes(27, 12, limit, 2, 1), at_limit, few_cls, few, alpha=list(np.linspace(0, 1, 9)))
    # a fold of one class: group 0 holds twenty rows of class 0 and nothing else
    order = np.argsort(y, kind="stable")
    one_class = np.empty(60, dtype=np.int64)
    one_class[order[:20]] = 0
    one_class[order[20:]] = 1 + np.arange(40) % 2
    refused(-1, "the training set of group 0 of 3 holds one class only", x, y, one_class)
    refused(-1, "the training set of group 0 of 3 holds one class only", sp.csc_matrix(x), y, one_class)
    # a width the library does not have
    with sa.option("wnewton_width", 512):
        refused(-1, "wnewton_width", x, y, fold)

    # what cv_wnewton_fits cannot express goes through the C ABI directly
    L = sa.load()
    xf, yf, f32 = np.asfortranarray(x), np.ascontiguousarray(y), np.ascontiguousarray(fold, dtype=np.int32)
    alphas, lam = np.array([0.5]), np.array([[0.1, 0.01]])

    def call(fold_arr=f32, n_groups=3, lam_arr=lam, y_arr=yf, **ctl_fields):
        ctl = _lib.Control()
        ctl.family, ctl.intercept, ctl.standardize, ctl.max_iter, ctl.tol, ctl.n_lambda, ctl.n_classes = 1, 1, 1, 100, 1e-7, 2, 1
        for k, v in ctl_fields.items():
            setattr(ctl, k, v)
        out = [np.zeros(3 * 2), np.zeros(3 * 2 * 4), np.zeros(3 * 2), np.zeros(3 * 2), np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3)]
        res = _lib.CvNewtonResult(*[_lib.dptr(a) for a in out])
        rc = L.sgdnet_cv_wnewton_dense(_lib.dptr(xf), 60, 4, _lib.dptr(y_arr), fold_arr.ctypes.data_as(C.POINTER(C.c_int32)), n_groups, 0,
                                       C.byref(ctl), 1, _lib.dptr(alphas), _lib.dptr(lam_arr), C.byref(res))
        return rc, L.sgdnet_last_error().decode()

    rc, msg = call(n_gpus=2)
    assert rc == -5 and msg.startswith("mode = wnewton needs one GPU"), msg
    rc, msg = call(debug=1)
    assert rc == -5 and msg.startswith("mode = wnewton needs debug = 0"), msg
    for family in (0, 2, 3):
        rc, msg = call(family=family)
        assert rc == -5 and msg.startswith("mode = wnewton needs family = binomial"), msg
    bad = f32.copy()
    bad[7] = 3
    rc, msg = call(fold_arr=bad)
    assert rc == -1 and "fold[7] = 3" in msg, msg
    rc, msg = call(n_groups=4)
    assert rc == -1 and "group 3 of 4 is empty" in msg, msg
    rc, msg = call(lam_arr=np.array([[0.1, -0.01]]))
    assert rc == -1 and "negative" in msg, msg
    rc, msg = call(y_arr=yf + 0.5)
    assert rc == -1 and "is not a class code" in msg, msg

    # sgdnet() and cv_sgdnet() do not learn the mode
    with pytest.raises(ValueError, match="mode must be one of 'exact', 'batched', 'auto', 'covariance'$"):
        sa.sgdnet(x, y, family="binomial", nlambda=3, mode="wnewton")
    with pytest.raises(ValueError, match="mode must be one of"):
        sa.cv_sgdnet(x, y, family="binomial", nfolds=3, nlambda=3, mode="wnewton")
    with pytest.raises(ValueError, match="fold_fits='batched' needs mode='covariance'"):
        sa.cv_sgdnet(x, y, family="binomial", nfolds=3, mode="wnewton", fold_fits="batched")


# ---- the inputs of the GPU test ----

def test_row_chunk_inputs_have_the_chunks_they_are_there_for():
    inputs = cr.row_chunk_inputs()
    x, y, foldid, sizes = inputs["two"]
    assert [int((foldid == v).sum()) for v in np.unique(foldid)] == sizes == [300, 200]
    # train_on = "fold": a job of two row chunks beside a job of one
    assert [cr.job_chunks(n_t, 1) for n_t in (300, 200)] == [2, 1] and cr.rows_per_chunk(300, 3) == 192
    assert [cr.job_chunks(500 - n_t, 1) for n_t in (300, 200)] == [1, 2]
    x, y, foldid, sizes = inputs["gap"]
    assert [int((foldid == v).sum()) for v in np.unique(foldid)] == sizes == [100, 200, 200]
    # train_on = "rest", the middle group: 100 rows below it and 200 above, two chunks of 192 local rows -- the first crosses
    assert cr.job_chunks(300, 1) == 2 and 100 < cr.rows_per_chunk(300, 3) < 300
    assert [cr.job_chunks(500 - n_t, 1) for n_t in sizes] == [2, 2, 2] and [cr.job_chunks(n_t, 1) for n_t in sizes] == [1, 1, 1]
    for name in inputs:                                               # every training set holds both classes
        x, y, foldid, _ = inputs[name]
        for train_on in ("fold", "rest"):
            assert all(0 < y[T].sum() < T.sum() for T in cr.training_sets(foldid, train_on))
    x, y, foldid = cr.leave_one_out_input()
    assert len(cr.training_sets(foldid, "rest")) * 3 == 270 > 256 and all(0 < y[T].sum() < 89 for T in cr.training_sets(foldid, "rest"))
    # the restatement of wide_row_chunks is the header's: its two static_asserts and the chunk rule's corners
    assert cr.wide_row_chunks(1 << 30, wr.LIMIT + 2) == 1 and cr.wide_row_chunks(1 << 30, 3) == 1024 and cr.wide_row_chunks(1, 3) == 1


@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("shape", cr.SHAPES[:-1])
def test_the_restatement_of_every_job_is_optimal(shape, train_on):
    """the CPU proof: KKT_BOUND on x[T], y[T] for every job and lambda, by the restatement with the driver's pooled centres"""
    n, p, G = shape
    x, y = tn.problem(n, p, False)
    foldid = cr.equal_folds(n, G)
    moments = cr.pooled_moments(x, foldid, train_on)
    for mix in cr.MIXES:
        lam = cr.lambdas_of(x, y, shape, mix)
        for j, T in enumerate(cr.training_sets(foldid, train_on)):
            a0, beta, info = cr.pooled_job_path(x, y, T, moments[j], lam, mix)
            assert info["codes"] == [0] * len(lam), (shape, train_on, mix, j, info)
            tn.assert_optimal(tn.numpy_kkt(a0, beta, x[T], y[T], lam, mix, True, True), lam, (shape, train_on, mix, j))


POOLED_WORST = []


@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("shape", [s for s in cr.SHAPES[:-1] if s[1] <= 256])
def test_pooled_centres_do_not_move_the_optimum(shape, train_on):
    sparse = False                                                    # (a sparse call is the dense call on the same matrix)
    n, p, G = shape
    x, y = tn.problem(n, p, sparse)
    foldid = cr.equal_folds(n, G)
    moments = cr.pooled_moments(x, foldid, train_on)
    worst = 0.0
    for mix in cr.MIXES:
        lam = cr.lambdas_of(x, y, shape, mix)
        for j, T in enumerate(cr.training_sets(foldid, train_on)):
            a_own, b_own, info_own = cr.job_path(x, y, T, lam, mix)
            a_all, b_all, info_all = cr.pooled_job_path(x, y, T, moments[j], lam, mix)
            assert not any(info_own["codes"]) and not any(info_all["codes"]), (shape, sparse, train_on, mix, j)
            scale = np.abs(b_own).max()
            worst = max(worst, np.abs(b_all - b_own).max() / scale, np.abs(a_all - a_own).max() / scale)
    POOLED_WORST.append(worst)
    print("pooled centres vs own centres: largest relative difference %.3g (over the cases so far %.3g)" % (worst, max(POOLED_WORST)))
    assert worst <= cr.SAME_OPTIMUM / 10, (shape, sparse, train_on, worst)


def test_the_rewritten_restatement_is_the_restatement():
    """with the set's own mean and variance passed in, pooled_job_path is numpy_wide_newton_path bit for bit"""
    x, y = tn.problem(37, 2, False)
    lam = cr.lambdas_of(x, y, (37, 2, 3), 0.5)
    T = np.ones(37, dtype=bool)
    a, b, _ = cr.job_path(x, y, T, lam, 0.5)
    a2, b2, _ = cr.pooled_job_path(x, y, T, (x.mean(axis=0), ((x - x.mean(axis=0)) ** 2).mean(axis=0)), lam, 0.5)
    assert a.tobytes() == a2.tobytes() and b.tobytes() == b2.tobytes()


def test_the_halving_input_halves_and_its_jobs_differ():
    """What tests/test_gpu_cv_wnewton.py relies on: in the restatement some job halves a step, the two jobs take different
    numbers of steps (so one round holds jobs at different lambdas), and every lambda converges.

    Measured when the test was written, own centres: job 0 takes 18 + 7 steps with 1 halving, job 1 takes 20 + 7 with 4;
    pooled centres: 18 + 7 with 1 and 19 + 7 with 1 -- at lambda = 1e-6 on nearly separable data a last-place difference in
    the centres moves the whole trajectory, which is why coefficients are not compared there.  The penalised objective is
    flat where the coefficients are not determined: its relative difference between the two restatements is at most 1.65e-12
    (job 1 at lambda = 1e-6; 1.3e-16 elsewhere).  cv_wnewton_reference.HALVING_OBJECTIVE_DIFFERENCE records it; the figures are
    printed."""
    x, y, foldid = cr.halving_input()
    H = cr.HALVING
    kw = dict(thresh=H["thresh"], maxit=H["maxit"])
    moments = cr.pooled_moments(x, foldid, "rest")
    totals, halvings, worst = [], [], 0.0
    for j, T in enumerate(cr.training_sets(foldid, "rest")):
        a_own, b_own, own = cr.job_path(x, y, T, H["lam"], H["mix"], **kw)
        a_all, b_all, pooled = cr.pooled_job_path(x, y, T, moments[j], H["lam"], H["mix"], **kw)
        assert own["codes"] == [0, 0] and pooled["codes"] == [0, 0], (j, own, pooled)
        totals.append((sum(own["steps"]), sum(pooled["steps"])))
        halvings.append((own["halvings"], pooled["halvings"]))
        f_own = cr.objective(a_own, b_own, x[T], y[T], H["lam"], H["mix"])
        f_all = cr.objective(a_all, b_all, x[T], y[T], H["lam"], H["mix"])
        worst = max(worst, (np.abs(f_all - f_own) / np.abs(f_own)).max())
    print("halving input: steps (own, pooled) per job", totals, "halvings", halvings, "objective difference %.3g" % worst)
    for k in (0, 1):                                                  # own centres, and the driver's
        assert max(h[k] for h in halvings) >= 1 and totals[0][k] != totals[1][k]
    # (another BLAS may round the trajectories differently: the record stands while the GPU test's bound covers what is measured)
    assert worst <= cr.HALVING_OBJECTIVE_BOUND
