"""mode="covariance" without a GPU: the Python surface, the constants of the three layers, and the numpy restatement
of the algorithm (tests/test_gpu_covariance.py: numpy_cd_path) that the GPU tests' inputs and bounds lean on."""
import os
import re

import numpy as np
import pytest

import test_gpu_covariance as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mode_strings():
    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    assert _lib.MODES == {"exact": 0, "batched": 1, "auto": 2, "covariance": 3}
    x = np.random.default_rng(0).standard_normal((20, 3))
    y = x[:, 0] + 1.0
    with pytest.raises(ValueError, match="mode must be one of"):
        sa.sgdnet(x, y, nlambda=3, mode="gram")
    if sa.load().sgdnet_device_count() == 0:
        # "covariance" passes the argument mapping and reaches the backend, which has no device to run on
        with pytest.raises(sa.SgdnetError) as e:
            sa.sgdnet(x, y, nlambda=3, mode="covariance")
        assert e.value.code == -2


def test_header_binding_and_package_agree():
    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sgdnet_hip.h")).read()
    assert int(re.search(r"#define SGDNET_MODE_COVARIANCE\s+(\d+)", hdr).group(1)) == _lib.MODES["covariance"] == 3
    assert int(re.search(r"#define SGDNET_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 6
    assert "sgdnet_covariance_max_features" in _lib.EXPORTS and "covariance_max_features" in sa.__all__
    pmax = sa.covariance_max_features()
    assert pmax == sa.load().sgdnet_covariance_max_features() == 198 and pmax >= 64
    # the LDS budget written next to the constant (csrc/covariance.hpp): triangle + three vectors in 160 KiB of doubles
    state = lambda p: p * (p + 1) // 2 + 3 * p                                               # noqa: E731
    assert state(pmax) <= 160 * 1024 // 8 < state(pmax + 1)
    shim = open(os.path.join(ROOT, "shim", "sgdnet_shim.c")).read()
    assert '"covariance") == 0) c->mode = SGDNET_MODE_COVARIANCE' in shim


@pytest.mark.parametrize("mix", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", tc.SHAPES[:-1])
def test_numpy_optimum_is_inside_the_bound(shape, sparse, mix):
    """The inputs of test_gpu_covariance.py::test_automatic_path_is_optimal: an optimum computed in plain f64 passes the
    same check, so the bound asks nothing of the device that the number format does not give.  (The widest shape is
    test_numpy_optimum_at_the_feature_limit.)"""
    check_numpy_optimum(shape[0], shape[1], sparse, mix, [(True, True), (False, False), (True, False), (False, True)])


@pytest.mark.parametrize("sparse", [False, True])
def test_numpy_optimum_at_the_feature_limit(sparse):
    import sgdnet_amd as sa
    check_numpy_optimum(300, sa.covariance_max_features(), sparse, 0.5, [(True, True)], nlambda=4)


def check_numpy_optimum(n, p, sparse, mix, settings, nlambda=20):
    x, y = tc.problem(n, p, sparse)
    for intercept, standardize in settings:
        lam = automatic_lambdas(x, y, mix, standardize, intercept, nlambda, 1e-2)
        a0, beta = tc.numpy_cd_path(x, y, lam, mix, standardize, intercept)
        k = tc.numpy_kkt(a0, beta, x, y, lam, mix, standardize, intercept)
        tc.assert_optimal(k, lam, (n, p, sparse, mix, intercept, standardize))


def automatic_lambdas(x, y, mix, standardize, intercept, nlambda, ratio):
    """regularization_path / lambda_max of the driver for a gaussian response (driver.cpp)."""
    import sgdnet_amd as sa
    xd = np.asarray(x.todense()) if hasattr(x, "todense") else x
    xc, xs = sa.feature_moments(x, standardize)
    lmax = np.abs(((xd - xc) / xs).T @ (y - y.mean())).max() / len(y) / max(mix, 0.001)
    return np.exp(np.linspace(np.log(lmax), np.log(lmax * ratio), nlambda))


def test_user_lambdas_and_degenerate_inputs_in_numpy():
    x, y = tc.problem(65, 17, False, seed=1)
    a0, beta = tc.numpy_cd_path(x, y, tc.NONMONOTONE, 0.5)
    tc.assert_optimal(tc.numpy_kkt(a0, beta, x, y, tc.NONMONOTONE, 0.5, True, True), np.array(tc.NONMONOTONE), "user lambdas")
    x, y = tc.problem(120, 6, False, seed=5)
    x[:, 5] = x[:, 1]
    x[:, 4] = 3.0
    lam = automatic_lambdas(x, y, 1.0, True, True, 8, 1e-2)
    a0, beta = tc.numpy_cd_path(x, y, lam, 1.0)
    assert (beta[4] == 0).all()
    tc.assert_optimal(tc.numpy_kkt(a0, beta, x, y, lam, 1.0, True, True), lam, "identical + constant columns")


@pytest.mark.parametrize("mix", [0.0, 0.3, 1.0])
def test_numpy_restatement_reproduces_sklearn(mix):
    """sklearn's ElasticNet minimises |y - X w|^2 / (2 n) + a r |w|_1 + a (1 - r) |w|^2 / 2; the driver's problem on the
    standardised features (kkt.py) is that with a r = mix lambda and a (1 - r) = (1 - mix) lambda / sd(y)."""
    sk = pytest.importorskip("sklearn.linear_model")
    x, y = tc.problem(65, 17, False, seed=1)
    lam = [0.4, 0.1, 0.02]
    a0, beta = tc.numpy_cd_path(x, y, lam, mix)
    xs = (x - x.mean(axis=0)) / x.std(axis=0)
    for l, (a0_l, b_l) in enumerate(zip(a0, beta.T)):
        l1, l2 = mix * lam[l], (1 - mix) * lam[l] / y.std()
        if mix == 0.0:
            ref = sk.Ridge(alpha=l2 * len(y), fit_intercept=False, tol=1e-14, solver="cholesky").fit(xs, y - y.mean()).coef_
        else:
            ref = sk.ElasticNet(alpha=l1 + l2, l1_ratio=l1 / (l1 + l2), fit_intercept=False, tol=1e-14,
                                max_iter=1_000_000).fit(xs, y - y.mean()).coef_
        assert np.abs(b_l * x.std(axis=0) - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
        assert abs(a0_l - (y.mean() - x.mean(axis=0) @ b_l)) <= 1e-12 * max(1.0, abs(y.mean()))


def test_oracle_distance_from_its_optimum_on_abalone(oracle):
    """Where ORACLE_REL_CHANGE of test_gpu_covariance.py comes from: the oracle's own coefficients move by this much
    between thresh and thresh / 100.  The numpy optimum is within 10 x that of the oracle's, as the GPU fit has to be."""
    ab = np.load(os.path.join(tc.GOLD, "abalone.npz"))
    kw = dict(family="gaussian", maxit=100000, seed=1, **tc.ABALONE)
    ref = oracle.fit(ab["x"], ab["y"], thresh=tc.ORACLE_THRESH, **kw)
    tight = oracle.fit(ab["x"], ab["y"], thresh=tc.ORACLE_THRESH / 100, **kw)
    scale = np.abs(tight["beta"]).max()
    change = np.abs(ref["beta"] - tight["beta"]).max() / scale
    print("oracle, abalone: change between thresh %g and thresh / 100, relative to max|beta|: %.3g" % (tc.ORACLE_THRESH, change))
    assert change <= tc.ORACLE_REL_CHANGE
    a0, beta = tc.numpy_cd_path(ab["x"], ab["y"], ref["lambda"], tc.ABALONE["alpha"])
    assert np.abs(beta - ref["beta"][0]).max() / scale <= tc.ORACLE_TOL
