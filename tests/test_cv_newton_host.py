"""Cross-validation in Newton mode (sgdnet_cv_newton_*, sa.cv_newton_fits, sa.cv_sgdnet_newton), the parts a CPU can check:
the three layers agree on the new names, the Python functions validate their arguments, the native entry points refuse
what they refuse before a device is looked for, and the inputs and the tolerance of tests/test_gpu_cv_newton.py are sound.

The tolerance measurement.  A job solves x[T], y[T] as a Newton problem about fixed centres m; the optimum (beta, a0) does
not depend on m, what the iteration reaches at a given thresh could.  newton_path_about() is numpy_newton_path of
tests/test_gpu_newton.py with the centres passed in; the same job is solved about T's own column means and about the means of
the whole data, at thresh = 1e-12, on every (shape, sparse, train_on, mix) of the GPU envelope test below p = 33.  The
relative difference of beta and a0 is asserted <= 1e-10 -- a decade under the 1e-9 (SAME_OPTIMUM) the GPU test holds a job
to against its separate fit -- and the largest is printed (1.8e-11 when the test was written)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import test_gpu_cv_covariance as tcv
import test_gpu_newton as tn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTRE_BOUND = 1e-10
ENVELOPE_BELOW_33 = [(37, 2, 3), (192, 14, 3), (195, 15, 3), (195, 16, 3)]      # tests/test_gpu_cv_newton.py: SHAPES with p < 33
MIXES = [0.0, 0.5, 1.0]
NLAMBDA = 8


def test_header_binding_and_package_agree():
    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sgdnet_hip.h")).read()
    assert int(re.search(r"#define SGDNET_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 6       # additions only
    for name in ("sgdnet_cv_newton_dense", "sgdnet_cv_newton_sparse"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.EXPORTS, name
    for name in ("cv_newton_fits", "cv_sgdnet_newton"):
        assert name in sa.__all__ and callable(getattr(sa, name)), name
    # the result struct, field for field
    body = re.search(r"typedef struct sgdnet_cv_newton_result \{(.*?)\} sgdnet_cv_newton_result;", hdr, re.S).group(1)
    fields = re.findall(r"double\*\s+(\w+);", body)
    assert fields == [f[0] for f in _lib.CvNewtonResult._fields_] == ["a0", "beta", "dev_ratio", "return_codes", "nulldev", "npasses", "steps",
                                                                      "halvings"]
    # the two CV entry points take the same arguments but for the result
    cov = re.search(r"int sgdnet_cv_covariance_dense\((.*?)\);", hdr, re.S).group(1)
    new = re.search(r"int sgdnet_cv_newton_dense\((.*?)\);", hdr, re.S).group(1)
    assert " ".join(cov.split()).replace("sgdnet_cv_cov_result", "sgdnet_cv_newton_result") == " ".join(new.split())
    # the workspace limit is a named constant whose value the header states
    newton_hpp = open(os.path.join(ROOT, "sgdnet_amd", "csrc", "newton.hpp")).read()
    assert re.search(r"kNewtonCvWorkspaceBytes = \(size_t\)1 << 30;", newton_hpp) and "above 1 GiB" in hdr


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
            sa.cv_newton_fits(x, y, fold, *args, **kw)
    with pytest.raises(ValueError, match="must match"):
        sa.cv_newton_fits(x, y, fold[:-1], 0.5, [0.1])
    with pytest.raises(ValueError, match="more than two classes"):
        sa.cv_newton_fits(x, np.arange(60) % 3, fold, 0.5, [0.1])
    with pytest.raises(ValueError, match="only one class"):
        sa.cv_newton_fits(x, np.ones(60), fold, 0.5, [0.1])
    for needle, kw in (("'separate' or 'batched'", dict(fold_fits="fused")), ("train_on must be", dict(train_on="others")),
                       ("nfolds > 2", dict(nfolds=2)), ("'arg' should be one of", dict(type_measure="r2")),
                       ("more folds than samples", dict(nfolds=61)),
                       ("need a list of lambdas", dict(alpha=[0.5, 1.0], lambda_=[0.1, 0.01]))):
        with pytest.raises(ValueError, match=needle):
            sa.cv_sgdnet_newton(x, y, **kw)
    with pytest.raises(TypeError):
        sa.cv_sgdnet_newton(x, y, mode="auto")                                     # the mode is not an argument: every fit is Newton's


def test_native_refusals_name_the_condition():
    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = (x[:, 0] + rng.standard_normal(60) > 0).astype(float)
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
    # leave-one-out of 300 rows at 198 features: 5 mixes fit the 1 GiB of workspace (newton.hpp), 8 do not
    big = rng.standard_normal((300, pm))
    refused(-5, "mode = newton needs the jobs' workspace within 1073741824 bytes", big, (big[:, 0] > 0).astype(float), np.arange(300),
            alpha=list(np.linspace(0, 1, 8)), train_on="rest")
    # a fold of one class: group 0 holds twenty rows of class 0 and nothing else
    order = np.argsort(y, kind="stable")
    one_class = np.empty(60, dtype=np.int64)
    one_class[order[:20]] = 0
    one_class[order[20:]] = 1 + np.arange(40) % 2
    refused(-1, "the training set of group 0 of 3 holds one class only", x, y, one_class)
    refused(-1, "the training set of group 0 of 3 holds one class only", sp.csc_matrix(x), y, one_class)

    # what cv_newton_fits cannot express goes through the C ABI directly
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
        rc = L.sgdnet_cv_newton_dense(_lib.dptr(xf), 60, 4, _lib.dptr(y_arr), fold_arr.ctypes.data_as(C.POINTER(C.c_int32)), n_groups, 0,
                                      C.byref(ctl), 1, _lib.dptr(alphas), _lib.dptr(lam_arr), C.byref(res))
        return rc, L.sgdnet_last_error().decode()

    rc, msg = call(n_gpus=2)
    assert rc == -5 and msg.startswith("mode = newton needs one GPU"), msg
    rc, msg = call(debug=1)
    assert rc == -5 and msg.startswith("mode = newton needs debug = 0"), msg
    for family in (0, 2, 3):
        rc, msg = call(family=family)
        assert rc == -5 and msg.startswith("mode = newton needs family = binomial"), msg
    bad = f32.copy()
    bad[7] = 3
    rc, msg = call(fold_arr=bad)
    assert rc == -1 and "fold[7] = 3" in msg, msg
    bad[7] = -1
    rc, msg = call(fold_arr=bad)
    assert rc == -1 and "fold[7] = -1" in msg, msg
    rc, msg = call(n_groups=4)
    assert rc == -1 and "group 3 of 4 is empty" in msg, msg
    rc, msg = call(lam_arr=np.array([[0.1, -0.01]]))
    assert rc == -1 and "negative" in msg, msg
    rc, msg = call(y_arr=yf + 0.5)
    assert rc == -1 and "is not a class code" in msg, msg


# ---- the tolerance measurement ----

def newton_path_about(m, x, y, lam, mix, **kw):
    """numpy_newton_path (tests/test_gpu_newton.py) with the fixed centres of the Newton problem passed in: the source of that
    function with the one line that chooses them replaced, so that the two cannot drift apart."""
    src = inspect.getsource(tn.numpy_newton_path)
    line = "m = mean if (standardize or intercept) else np.zeros(p)"
    assert src.count(line) == 1 and src.count("def numpy_newton_path(") == 1
    src = src.replace(line, "m = np.asarray(CENTRES, dtype=float)").replace("def numpy_newton_path(", "def about(")
    scope = dict(vars(tn), CENTRES=m)
    exec(src, scope)
    return scope["about"](x, y, lam, mix, **kw)


@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", ENVELOPE_BELOW_33)
def test_the_centres_of_the_newton_problem_do_not_move_its_optimum(shape, sparse, train_on):
    n, p, G = shape
    x, y = tn.problem(n, p, sparse)
    xd = np.asarray(x.todense()) if sparse else x
    whole = xd.mean(axis=0)
    worst = 0.0
    for mix in MIXES:
        lam = tn.automatic_lambdas(x, y, mix, True, NLAMBDA, 1e-2)
        for j, T in enumerate(tcv.training_sets(tcv.equal_folds(n, G), train_on)):
            xT, yT = xd[T], y[T]
            assert min(yT.sum(), len(yT) - yT.sum()) >= 2
            a_own, b_own, info_own = tn.numpy_newton_path(xT, yT, lam, mix, thresh=1e-12)
            a_all, b_all, info_all = newton_path_about(whole, xT, yT, lam, mix, thresh=1e-12)
            assert not any(info_own["codes"]) and not any(info_all["codes"]), (shape, sparse, train_on, mix, j)     # every lambda converged
            err = max(np.abs(b_all - b_own).max() / np.abs(b_own).max(), np.abs(a_all - a_own).max() / max(1.0, np.abs(a_own).max()))
            worst = max(worst, err)
            assert err <= CENTRE_BOUND, (shape, sparse, train_on, mix, j, err)
    print("own centres vs whole-data centres: largest relative difference %.3g" % worst)


def test_the_rewritten_restatement_is_the_restatement():
    """about T's own means newton_path_about() is numpy_newton_path, bit for bit"""
    x, y = tn.problem(37, 2, False)
    lam = tn.automatic_lambdas(x, y, 0.5, True, NLAMBDA, 1e-2)
    a, b, _ = tn.numpy_newton_path(x, y, lam, 0.5)
    a2, b2, _ = newton_path_about(x.mean(axis=0), x, y, lam, 0.5)
    assert a.tobytes() == a2.tobytes() and b.tobytes() == b2.tobytes()


def test_numpy_converges_on_a_job_at_the_feature_limit():
    """one job of the (1800, 198, 3) shape with lambda down to 5e-2 lambda_max: the GPU test at the LDS limit asks nothing
    the restatement cannot do"""
    import sgdnet_amd as sa
    n, p, G = 1800, sa.newton_max_features(), 3
    x, y = tn.problem(n, p, False)
    lam = tn.automatic_lambdas(x, y, 0.5, True, NLAMBDA, tn.ratio_for(p))
    T = tcv.training_sets(tcv.equal_folds(n, G), "fold")[0]
    a0, beta, info = tn.numpy_newton_path(x[T], y[T], lam, 0.5)
    assert info["codes"] == [0] * NLAMBDA, info
    tn.assert_optimal(tn.numpy_kkt(a0, beta, x[T], y[T], lam, 0.5, True, True), lam, "one job at p = 198")
