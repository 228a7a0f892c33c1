"""sa.sgdnet_newton without a GPU: the Python surface, the constants of the three layers, and the numpy restatement of
the algorithm (tests/test_gpu_newton.py: numpy_newton_path) that the GPU tests' inputs and bounds lean on."""
import os
import re

import numpy as np
import pytest

import test_gpu_newton as tn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_package_agree():
    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sgdnet_hip.h")).read()
    assert int(re.search(r"#define SGDNET_MODE_NEWTON\s+(\d+)", hdr).group(1)) == _lib.MODE_NEWTON == 4
    assert int(re.search(r"#define SGDNET_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 6
    assert "int sgdnet_newton_max_features(void);" in hdr
    assert "sgdnet_newton_max_features" in _lib.EXPORTS
    assert "sgdnet_newton" in sa.__all__ and "newton_max_features" in sa.__all__
    # sgdnet() keeps its modes: the new one has its own function
    assert _lib.MODES == {"exact": 0, "batched": 1, "auto": 2, "covariance": 3}
    pmax = sa.newton_max_features()
    assert pmax == sa.load().sgdnet_newton_max_features() == 198
    # the LDS budget written next to the constant (csrc/newton.hpp): with P = p + 1 coordinates, the triangle of H and two
    # vectors in 160 KiB of doubles
    state = lambda p: (p + 1) * (p + 2) // 2 + 2 * (p + 1)                                   # noqa: E731
    assert state(pmax) <= 160 * 1024 // 8 < state(pmax + 1)
    shim = open(os.path.join(ROOT, "shim", "sgdnet_shim.c")).read()
    assert '"newton") == 0) c->mode = SGDNET_MODE_NEWTON' in shim
    newton_hpp = open(os.path.join(ROOT, "sgdnet_amd", "csrc", "newton.hpp")).read()
    for name, value in (("kNewtonMaxHalvings", tn.MAX_HALVINGS), ("kNewtonObjectiveSlack", tn.OBJECTIVE_SLACK), ("kNewtonMaxSweeps", tn.MAX_SWEEPS),
                        ("kNewtonNegligible", tn.NEGLIGIBLE)):
        assert eval(re.search(name + r" = ([0-9.e+* -]+);", newton_hpp).group(1)) == value, name


def test_no_device_and_argument_checks():
    import sgdnet_amd as sa
    x = np.random.default_rng(0).standard_normal((20, 3))
    y = (x[:, 0] > 0).astype(float)
    with pytest.raises(ValueError, match="mode must be one of 'exact', 'batched', 'auto', 'covariance'$"):
        sa.sgdnet(x, y, family="binomial", nlambda=3, mode="newton")
    # sgdnet()'s validation and its messages
    with pytest.raises(ValueError, match="more than two classes in response"):
        sa.sgdnet_newton(x, np.arange(20) % 3, nlambda=3)
    with pytest.raises(ValueError, match="elastic net mixing parameter"):
        sa.sgdnet_newton(x, y, alpha=1.5)
    if sa.load().sgdnet_device_count() == 0:
        # the call passes the argument mapping and reaches the backend, which has no device to run on
        with pytest.raises(sa.SgdnetError) as e:
            sa.sgdnet_newton(x, y, nlambda=3)
        assert e.value.code == -2


def check_numpy_optimum(n, p, sparse, mix, settings):
    x, y = tn.problem(n, p, sparse)
    for intercept, standardize in settings:
        lam = tn.automatic_lambdas(x, y, mix, standardize, tn.NLAMBDA, tn.ratio_for(p))
        a0, beta, info = tn.numpy_newton_path(x, y, lam, mix, standardize, intercept)
        assert not any(info["codes"]), info
        k = tn.numpy_kkt(a0, beta, x, y, lam, mix, standardize, intercept)
        print("halvings %d, outer steps %s" % (info["halvings"], info["steps"]))
        tn.assert_optimal(k, lam, (n, p, sparse, mix, intercept, standardize))


@pytest.mark.parametrize("mix", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", tn.SHAPES[:-1])
def test_numpy_optimum_is_inside_the_bound(shape, sparse, mix):
    """The inputs of test_gpu_newton.py::test_automatic_path_is_optimal: an optimum computed in plain f64 by the same
    algorithm passes the same check, so the bound asks nothing of the device that the number format does not give.
    (The widest shape is test_numpy_optimum_at_the_feature_limit.)"""
    check_numpy_optimum(shape[0], shape[1], sparse, mix, tn.SETTINGS)


@pytest.mark.parametrize("mix", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("sparse", [False, True])
def test_numpy_optimum_at_the_feature_limit(sparse, mix):
    import sgdnet_amd as sa
    check_numpy_optimum(600, sa.newton_max_features(), sparse, mix, [(True, True)])


def test_user_lambdas_and_degenerate_inputs_in_numpy():
    x, y = tn.problem(65, 16, False, seed=1)
    a0, beta, info = tn.numpy_newton_path(x, y, tn.NONMONOTONE, 0.5)
    assert not any(info["codes"])
    tn.assert_optimal(tn.numpy_kkt(a0, beta, x, y, tn.NONMONOTONE, 0.5, True, True), np.array(tn.NONMONOTONE), "user lambdas")
    x, y = tn.problem(120, 6, False, seed=5)
    x[:, 5] = x[:, 1]
    x[:, 4] = 3.0
    lam = tn.automatic_lambdas(x, y, 1.0, True, 8, 1e-2)
    a0, beta, info = tn.numpy_newton_path(x, y, lam, 1.0)
    assert (beta[4] == 0).all() and not any(info["codes"])
    tn.assert_optimal(tn.numpy_kkt(a0, beta, x, y, lam, 1.0, True, True), lam, "identical + constant columns")


@pytest.mark.parametrize("mix", [0.0, 0.3, 1.0])
def test_numpy_restatement_reproduces_sklearn(mix):
    """sklearn's LogisticRegression minimises C sum_i loss_i + r |w|_1 + (1 - r) |w|^2 / 2 with an unpenalised intercept;
    the driver's problem on the standardised features (kkt.py) is that divided by n C with 1 / (n C) = lambda, r = mix."""
    sk = pytest.importorskip("sklearn.linear_model")
    x, y = tn.problem(65, 16, False, seed=1)
    lam = [0.08, 0.02, 0.005]
    a0, beta, _ = tn.numpy_newton_path(x, y, lam, mix)
    xs = (x - x.mean(axis=0)) / x.std(axis=0)
    for l, (a0_l, b_l) in enumerate(zip(a0, beta.T)):
        kw = dict(C=1.0 / (len(y) * lam[l]), fit_intercept=True, tol=1e-12, max_iter=1_000_000)
        if mix == 0.0:
            ref = sk.LogisticRegression(penalty="l2", solver="lbfgs", **kw).fit(xs, y)
        else:
            ref = sk.LogisticRegression(penalty="elasticnet", l1_ratio=mix, solver="saga", **kw).fit(xs, y)
        w = b_l * x.std(axis=0)
        print("mix %g lambda %g: max coefficient difference %.3g" % (mix, lam[l], np.abs(w - ref.coef_[0]).max()))
        # sklearn's own stopping rule (lbfgs: projected gradient, saga: max change of the coefficients) sets the agreement
        assert np.abs(w - ref.coef_[0]).max() <= 1e-5 * max(1.0, np.abs(ref.coef_).max())
        assert abs(a0_l + x.mean(axis=0) @ b_l - ref.intercept_[0]) <= 1e-5 * max(1.0, abs(ref.intercept_[0]))


def test_oracle_distance_from_its_optimum_on_abalone(oracle):
    """Where ORACLE_REL_CHANGE of test_gpu_newton.py comes from: the oracle's own coefficients move by this much between
    thresh and thresh / 100.  The numpy optimum is within 10 x that of the oracle's, as the GPU fit has to be."""
    x, y = tn.abalone_binomial()
    kw = dict(family="binomial", maxit=100000, seed=1, **tn.ABALONE)
    ref = oracle.fit(x, y, thresh=tn.ORACLE_THRESH, **kw)
    tight = oracle.fit(x, y, thresh=tn.ORACLE_THRESH / 100, **kw)
    scale = np.abs(tight["beta"]).max()
    change = np.abs(ref["beta"] - tight["beta"]).max() / scale
    print("oracle, binomial abalone: change between thresh %g and thresh / 100, relative to max|beta|: %.3g" % (tn.ORACLE_THRESH, change))
    assert change <= tn.ORACLE_REL_CHANGE
    a0, beta, info = tn.numpy_newton_path(x, y, ref["lambda"], tn.ABALONE["alpha"])
    assert not any(info["codes"])
    assert np.abs(beta - ref["beta"][0]).max() / scale <= tn.ORACLE_TOL
    # intercepts below lambda_max only: there the oracle's stopping rule (coefficients only, all zero) leaves ITS
    # intercept short of its optimum
    assert np.abs(a0[1:] - ref["a0"][0, 1:]).max() <= tn.ORACLE_TOL * max(1.0, np.abs(ref["a0"]).max())
