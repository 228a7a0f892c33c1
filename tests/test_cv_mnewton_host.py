"""Cross-validation in multinomial Newton mode (sgdnet_cv_mnewton_*, sa.cv_mnewton_fits, sa.cv_sgdnet_mnewton), the parts a
CPU can check: the three layers agree on the new names, the Python functions validate their arguments, the native entry
points refuse what they refuse before a device is looked for, and the inputs and the tolerance of
tests/test_gpu_cv_mnewton.py are sound.

The tolerance measurement.  A job solves x[T], y[T] as a Newton problem about fixed centres m; the optimum (beta, a0) does not
depend on m, what the iteration reaches at a given thresh could.  A separate fit forms m on the device, the batched call on
the host (tests/cv_mnewton_reference.py: device_order_centres, host_order_centres): a perturbation of the means of rounding
size.  mnewton_path_about() solves the same job about both, at thresh = 1e-12, on every (shape, sparse, train_on, mix) of the
GPU envelope's small shapes.  The relative difference of beta and a0 is printed per case; the largest was 4.91e-15 when the test
was written (the centres themselves differ by up to 7.8e-16), and CENTRE_BOUND = 5e-14 pins 10 x that.  It is far below 1e-10,
so SAME_OPTIMUM, what the GPU test holds a job to against its separate fit, stays the project's 1e-9
(tests/test_gpu_cv_covariance.py), as it did for the binomial cross-validation; it would have been 10 x the measured value
otherwise."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import cv_mnewton_reference as ref
import test_gpu_cv_covariance as tcv
import test_gpu_mnewton as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTRE_BOUND, SAME_OPTIMUM = ref.CENTRE_BOUND, ref.SAME_OPTIMUM
assert CENTRE_BOUND <= 1e-10 and SAME_OPTIMUM == tcv.SAME_OPTIMUM == 1e-9       # (10 x the measured value had it been larger)


def test_header_binding_and_package_agree():
    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sgdnet_hip.h")).read()
    assert int(re.search(r"#define SGDNET_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 6       # additions only
    for name in ("sgdnet_cv_mnewton_dense", "sgdnet_cv_mnewton_sparse"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.EXPORTS and hasattr(sa.load(), name), name
    for name in ("cv_mnewton_fits", "cv_sgdnet_mnewton"):
        assert name in sa.__all__ and callable(getattr(sa, name)), name
    # the result struct, field for field
    body = re.search(r"typedef struct sgdnet_cv_mnewton_result \{(.*?)\} sgdnet_cv_mnewton_result;", hdr, re.S).group(1)
    fields = re.findall(r"double\*\s+(\w+);", body)
    assert fields == [f[0] for f in _lib.CvMNewtonResult._fields_] == ["a0", "beta", "dev_ratio", "return_codes", "nulldev", "npasses", "steps",
                                                                       "halvings"]
    # the entry points take the arguments of the binomial ones but for the result
    for form in ("dense", "sparse"):
        old = re.search(r"int sgdnet_cv_newton_%s\((.*?)\);" % form, hdr, re.S).group(1)
        new = re.search(r"int sgdnet_cv_mnewton_%s\((.*?)\);" % form, hdr, re.S).group(1)
        assert " ".join(old.split()).replace("sgdnet_cv_newton_result", "sgdnet_cv_mnewton_result") == " ".join(new.split())
    # the workspace limit is the binomial cross-validation's named constant, whose value the header states
    mnewton_hpp = open(os.path.join(ROOT, "sgdnet_amd", "csrc", "mnewton.hpp")).read()
    assert "kNewtonCvWorkspaceBytes" in mnewton_hpp and "above 1 GiB" in hdr.split("sgdnet_cv_newton_sparse(")[-1]


def test_python_argument_checks():
    import sgdnet_amd as sa
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = np.digitize(x[:, 0] + rng.standard_normal(60), [-0.5, 0.5])
    fold = np.arange(60) % 3
    for needle, args, kw in (("one array per alpha", ([0.5, 1.0], [[0.1, 0.01]]), {}),
                             ("must be positive", (0.5, [0.1, -0.01]), {}),
                             ("train_on must be", (0.5, [0.1]), dict(train_on="others")),
                             ("must be in \\[0, 1\\]", (1.5, [0.1]), {}),
                             ("cannot be negative", (0.5, [0.1]), dict(thresh=-1.0)),
                             ("negative or zero", (0.5, [0.1]), dict(maxit=0)),
                             ("must be logical", (0.5, [0.1]), dict(intercept=1))):
        with pytest.raises(ValueError, match=needle):
            sa.cv_mnewton_fits(x, y, fold, *args, **kw)
    with pytest.raises(ValueError, match="must match"):
        sa.cv_mnewton_fits(x, y, fold[:-1], 0.5, [0.1])
    with pytest.raises(ValueError, match="must be one-dimensional"):
        sa.cv_mnewton_fits(x, np.eye(3)[y], fold, 0.5, [0.1])
    with pytest.raises(ValueError, match="only one class"):
        sa.cv_mnewton_fits(x, np.ones(60), fold, 0.5, [0.1])
    for needle, kw in (("'separate' or 'batched'", dict(fold_fits="fused")), ("train_on must be", dict(train_on="others")),
                       ("nfolds > 2", dict(nfolds=2)), ("'arg' should be one of", dict(type_measure="auc")),
                       ("more folds than samples", dict(nfolds=61)),
                       ("need a list of lambdas", dict(alpha=[0.5, 1.0], lambda_=[0.1, 0.01]))):
        with pytest.raises(ValueError, match=needle):
            sa.cv_sgdnet_mnewton(x, y, **kw)
    with pytest.raises(TypeError):
        sa.cv_sgdnet_mnewton(x, y, mode="auto")                                    # the mode is not an argument: every fit is mnewton's
    with pytest.raises(ValueError, match="mode must be one of"):
        sa.cv_sgdnet(x, y, family="multinomial", nfolds=3, mode="mnewton")         # cv_sgdnet() does not learn the mode


def test_native_refusals_name_the_condition():
    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = np.digitize(x[:, 0] + rng.standard_normal(60), [-0.5, 0.5]).astype(float)
    fold = np.arange(60) % 3
    ref.folds(fold, y, 3)

    def refused(code, needle, xx, yy, ff, alpha=0.5, nlambda=2, **kw):
        lam = list(np.geomspace(0.1, 0.01, nlambda))
        with pytest.raises(sa.SgdnetError) as e:
            sa.cv_mnewton_fits(xx, yy, ff, alpha, [lam] * np.size(alpha) if np.ndim(alpha) else lam, **kw)
        assert e.value.code == code and needle in str(e.value), str(e.value)

    three = np.arange(30) % 3
    wide = rng.standard_normal((30, sa.mnewton_max_features(3) + 1))
    refused(-5, "mode = mnewton needs no more features than sgdnet_mnewton_max_features(n_classes)", wide, three, np.arange(30) // 10)
    refused(-5, "mode = mnewton needs no more features", sp.csc_matrix(wide), three, np.arange(30) // 10)
    assert sa.mnewton_max_features(100) == 0
    refused(-5, "mode = mnewton needs 2 to 99 classes", rng.standard_normal((200, 1)), np.arange(200) % 100, np.arange(200) // 100)
    # leave-one-out of 300 rows at K = 3 and its 65 features, 100 lambdas: 4 mixes fit the 1 GiB of workspace (mnewton.hpp), 8 do not
    big = rng.standard_normal((300, sa.mnewton_max_features(3)))
    refused(-5, "mode = mnewton needs the jobs' workspace within 1073741824 bytes", big, np.arange(300) % 3, np.arange(300),
            alpha=list(np.linspace(0, 1, 8)), train_on="rest", nlambda=100)
    # jobs x class pairs ride in a grid dimension: 600 jobs x 120 pairs at K = 15
    many = rng.standard_normal((300, 2))
    refused(-5, "mode = mnewton needs no more than 65535 jobs and 65535 jobs x class pairs", many, np.arange(300) % 15, np.arange(300),
            alpha=[0.5, 1.0], train_on="rest")
    # the dense copy of a sparse x: 1.4 million rows x 98 features x 8 bytes
    tall = sp.csc_matrix((np.ones(2), (np.array([0, 1]), np.array([0, 1]))), shape=(1_400_000, 98))
    refused(-5, "mode = mnewton needs the dense copy of a sparse x", tall, np.arange(1_400_000) % 2, np.arange(1_400_000) % 3)
    # a training set without a class: group 0 holds the rows of class 0 and nothing else
    order = np.argsort(y, kind="stable")
    first = int((y == 0).sum())
    missing = np.empty(60, dtype=np.int64)
    missing[order[:first]] = 0
    missing[order[first:]] = 1 + np.arange(60 - first) % 2
    refused(-1, "the training set of group 0 of 3 holds no row of class 1", x, y, missing)
    refused(-1, "the training set of group 0 of 3 holds no row of class 1", sp.csc_matrix(x), y, missing)
    refused(-1, "the training set of group 0 of 3 holds no row of class 0", x, y, missing, train_on="rest")     # (the other two groups)

    # what cv_mnewton_fits cannot express goes through the C ABI directly
    L = sa.load()
    xf, yf, f32 = np.asfortranarray(x), np.ascontiguousarray(y), np.ascontiguousarray(fold, dtype=np.int32)
    alphas, lam = np.array([0.5]), np.array([[0.1, 0.01]])

    def call(fold_arr=f32, n_groups=3, lam_arr=lam, y_arr=yf, **ctl_fields):
        ctl = _lib.Control()
        ctl.family, ctl.intercept, ctl.standardize, ctl.max_iter, ctl.tol, ctl.n_lambda, ctl.n_classes = 2, 1, 1, 100, 1e-7, 2, 3
        for k, v in ctl_fields.items():
            setattr(ctl, k, v)
        out = [np.zeros(3 * 2 * 3), np.zeros(3 * 2 * 4 * 3), np.zeros(3 * 2), np.zeros(3 * 2), np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3)]
        res = _lib.CvMNewtonResult(*[_lib.dptr(a) for a in out])
        rc = L.sgdnet_cv_mnewton_dense(_lib.dptr(xf), 60, 4, _lib.dptr(y_arr), fold_arr.ctypes.data_as(C.POINTER(C.c_int32)), n_groups, 0,
                                       C.byref(ctl), 1, _lib.dptr(alphas), _lib.dptr(lam_arr), C.byref(res))
        return rc, L.sgdnet_last_error().decode()

    rc, msg = call(n_gpus=2)
    assert rc == -5 and msg.startswith("mode = mnewton needs one GPU"), msg
    rc, msg = call(debug=1)
    assert rc == -5 and msg.startswith("mode = mnewton needs debug = 0"), msg
    for family in (0, 1, 3):
        rc, msg = call(family=family)
        assert rc == -5 and msg.startswith("mode = mnewton needs family = multinomial"), msg
    for K in (1, 0, 100):
        rc, msg = call(n_classes=K)
        assert rc == -5 and msg.startswith("mode = mnewton needs 2 to 99 classes"), msg
    rc, msg = call(type_multinomial=1)
    assert rc == -5 and msg.startswith("mode = mnewton needs the ungrouped penalty"), msg
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
    assert rc == -1 and "is not a class code in 0..2" in msg, msg
    rc, msg = call(y_arr=np.where(yf == 2, 3.0, yf))
    assert rc == -1 and "is not a class code in 0..2" in msg, msg


# ---- the tolerance measurement ----

def test_the_rewritten_restatement_is_the_restatement():
    """about the centres numpy_mnewton_path chooses, mnewton_path_about() is numpy_mnewton_path, bit for bit"""
    x, y = tm.problem(45, 2, 3)
    lam = ref.lambdas(x, y, 3, 0.5)
    a, b, d, _ = tm.numpy_mnewton_path(x, y, 3, lam, 0.5)
    a2, b2, d2, _ = ref.mnewton_path_about(x.mean(axis=0), x, y, 3, lam, 0.5)
    assert a.tobytes() == a2.tobytes() and b.tobytes() == b2.tobytes() and d.tobytes() == d2.tobytes()


@pytest.mark.parametrize("train_on", ["fold", "rest"])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", ref.SMALL_SHAPES)
def test_where_the_centres_are_formed_does_not_move_the_optimum(shape, sparse, train_on):
    n, p, K, G = shape
    x, y = tm.problem(n, p, K, sparse)
    xd = tm.dense(x)
    foldid = ref.equal_folds(n, G, y, K)
    worst = shift = 0.0
    for mix in ref.MIXES:
        assert ref.coefficients_are_unique(mix, K)
        lam = ref.lambdas(x, y, K, mix)
        for value, T in zip(np.unique(foldid), tcv.training_sets(foldid, train_on)):
            xT, yT = xd[T], y[T]
            on_device, on_host = ref.device_order_centres(xT), ref.host_order_centres(xd, foldid, value, train_on)
            shift = max(shift, np.abs(on_host - on_device).max())
            a_dev, b_dev, _, info_dev = ref.mnewton_path_about(on_device, xT, yT, K, lam, mix, thresh=1e-12)
            a_host, b_host, _, info_host = ref.mnewton_path_about(on_host, xT, yT, K, lam, mix, thresh=1e-12)
            assert not any(info_dev["codes"]) and not any(info_host["codes"]), (shape, sparse, train_on, mix, value)     # every lambda converged
            err = ref.relative_distance(a_host, b_host, a_dev, b_dev)
            worst = max(worst, err)
            assert err <= CENTRE_BOUND, (shape, sparse, train_on, mix, value, err)
    assert 0.0 < shift < 1e-13                                                       # a perturbation, and of rounding size
    print("host-order vs device-order centres (they differ by up to %.3g): largest relative difference of the optimum %.3g" % (shift, worst))


# ---- the pace case of the GPU test is chosen here ----

@pytest.mark.parametrize("train_on", ["fold", "rest"])
def test_the_jobs_of_the_pace_case_need_different_numbers_of_steps(train_on):
    S = ref.STEEP
    x, y = ref.steep_problem(False)
    foldid = ref.equal_folds(S["n"], S["folds"], y, S["K"], seed=S["fold_seed"])
    ref.folds(foldid, ref.steep_problem(True)[1], S["K"])
    steps = []
    for mix in S["mixes"]:
        for T in tcv.training_sets(foldid, train_on):
            a0, beta, _, info = tm.numpy_mnewton_path(x[T], y[T], S["K"], ref.STEEP_LAMBDAS, mix)
            assert info["codes"] == [0] * len(ref.STEEP_LAMBDAS), info
            tm.assert_optimal(tm.numpy_kkt(a0, beta, x[T], y[T], np.array(ref.STEEP_LAMBDAS), mix, True, True), np.array(ref.STEEP_LAMBDAS),
                              ("pace", train_on, mix))
            steps.append(sum(info["steps"]))
    print("outer steps per job", steps)
    assert len(set(steps)) > 1, steps


def test_the_inputs_of_the_gpu_test_hold_every_class_in_every_training_set():
    import sgdnet_amd as sa
    for n, p, K, G in ref.SHAPES + ref.LIMIT_SHAPES:
        for sparse in (False, True):
            for seed, fold_seed in ((0, 0), (1, 3)):          # the envelope; intercept x standardize
                _, y = tm.problem(n, p or sa.mnewton_max_features(K), K, sparse, seed=seed)
                ref.equal_folds(n, G, y, K, seed=fold_seed)
