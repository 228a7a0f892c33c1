"""sa.sgdnet_mcovariance without a GPU: the constants of the three layers, the LDS budget, and the numpy restatement of
the algorithm (tests/test_gpu_mcovariance.py: numpy_block_cd_path) that the GPU tests' inputs and bounds lean on.

Measured (plain f64, tol = 1e-13): the worst KKT ratio of the restatement's optimum is 5.7e-12 over the five small shapes
x 3 mixes x dense / sparse x 4 settings and 2.4e-12 at the two feature-limit shapes, the worst intercept residual
1.3e-13 lambda, and the quadratic form's dev_ratio is within 1e-15 of the residuals'; the bounds asked of the device are
1e-8 and 1e-10.  The oracle's distances are in test_gpu_mcovariance.py (ORACLE_*)."""
import os
import re

import numpy as np
import pytest

import test_gpu_mcovariance as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_DOUBLES = 160 * 1024 // 8
LIMITS = {1: 198, 2: 195, 3: 193, 5: 187, 10: 174, 16: 159, 32: 127, 64: 86, 95: 64, 96: 63}


def state_doubles(p, K):
    return p * (p + 1) // 2 + 3 * p * K


def max_features(K):
    """sgdnet_mcovariance_max_features: through the library where it loads, else restated from covariance.hpp's text."""
    try:
        import sgdnet_amd as sa
        return sa.mcovariance_max_features(K)
    except OSError:
        # (covariance.hpp's mcov_max_features at the K of LIMITS, from the compiled header: test_direct_plan_host.py)
        if K < 1 or state_doubles(1, K) > LDS_DOUBLES:
            return 0
        p = 1
        while state_doubles(p + 1, K) <= LDS_DOUBLES:
            p += 1
        return p


def test_header_binding_package_and_shim_agree():
    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sgdnet_hip.h")).read()
    assert int(re.search(r"#define SGDNET_MODE_MCOVARIANCE\s+(\d+)", hdr).group(1)) == _lib.MODE_MCOVARIANCE == 5
    assert int(re.search(r"#define SGDNET_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 6
    assert re.search(r"int sgdnet_mcovariance_max_features\(int n_responses\);", hdr)
    assert "sgdnet_mcovariance_max_features" in _lib.EXPORTS
    assert "sgdnet_mcovariance" in sa.__all__ and "mcovariance_max_features" in sa.__all__
    assert _lib.MODES == {"exact": 0, "batched": 1, "auto": 2, "covariance": 3}      # sgdnet(mode=...) does not reach mode 5
    shim = open(os.path.join(ROOT, "shim", "sgdnet_shim.c")).read()
    assert '"mcovariance") == 0) c->mode = SGDNET_MODE_MCOVARIANCE' in shim
    # (what the plan refuses of this mode, rung by rung and byte for byte: test_direct_plan_host.py)


def test_mode_string_is_not_one_of_sgdnet():
    import sgdnet_amd as sa
    x = np.random.default_rng(0).standard_normal((20, 3))
    y = np.column_stack([x[:, 0] + 1.0, x[:, 1]])
    with pytest.raises(ValueError, match="mode must be one of"):
        sa.sgdnet(x, y, family="mgaussian", nlambda=3, mode="mcovariance")
    if sa.load().sgdnet_device_count() == 0:
        # sgdnet_mcovariance passes the argument mapping and reaches the backend, which has no device to run on
        with pytest.raises(sa.SgdnetError) as e:
            sa.sgdnet_mcovariance(x, y, nlambda=3)
        assert e.value.code == -2


@pytest.mark.parametrize("K", sorted(LIMITS))
def test_feature_limit_is_the_lds_budget(K):
    p = max_features(K)
    assert p == LIMITS[K]
    assert state_doubles(p, K) <= LDS_DOUBLES < state_doubles(p + 1, K)


def test_feature_limit_where_nothing_fits():
    assert max_features(0) == 0 and max_features(-3) == 0
    assert max_features(6826) == 1 and max_features(6827) == 0 and max_features(2 ** 31 - 1) == 0
    # one response: the budget of mode = covariance
    import sgdnet_amd as sa
    assert max_features(1) == sa.covariance_max_features()


def automatic_lambdas(x, y, mix, standardize, nlambda, ratio, standardize_response=False):
    """regularization_path / lambda_max of the driver for mgaussian (driver.cpp): the largest row norm of X~'(Y - mean) / n."""
    import sgdnet_amd as sa
    xd, yd = tm.dense(x), tm.preprocessed_response(y, standardize_response)
    xc, xs = sa.feature_moments(x, standardize)
    c = ((xd - xc) / xs).T @ (yd - yd.mean(axis=0)) / len(yd)
    lmax = np.sqrt((c ** 2).sum(axis=1)).max() / max(mix, 0.001)
    return np.exp(np.linspace(np.log(lmax), np.log(lmax * ratio), nlambda))


def check_numpy_optimum(n, p, K, sparse, mix, settings, nlambda=20, standardize_response=False, seed=0):
    x, y = tm.problem(n, p, K, sparse, seed=seed)
    for intercept, standardize in settings:
        lam = automatic_lambdas(x, y, mix, standardize, nlambda, 1e-2, standardize_response)
        a0, beta, dev = tm.numpy_block_cd_path(x, y, lam, mix, standardize, intercept, standardize_response)
        k = tm.numpy_kkt(a0, beta, x, y, lam, mix, standardize, intercept, standardize_response)
        tm.assert_optimal(k, lam, (n, p, K, sparse, mix, intercept, standardize))
        # the quadratic form the driver reports the deviance from, against the residuals themselves
        ref = tm.numpy_dev_ratio(a0, beta, x, y, standardize, intercept, standardize_response)
        print("quadratic form vs residuals: dev_ratio differs by %.3g" % np.abs(dev - ref).max())
        assert np.abs(dev - ref).max() <= tm.DEV_TOL


@pytest.mark.parametrize("mix", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", tm.SMALL_SHAPES)
def test_numpy_optimum_is_inside_the_bound(shape, sparse, mix):
    """The inputs of test_gpu_mcovariance.py::test_automatic_path_is_optimal: an optimum computed in plain f64 passes the
    same checks, so the bounds ask nothing of the device that the number format does not give."""
    check_numpy_optimum(*shape, sparse, mix, tm.SETTINGS)


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", tm.LIMIT_SHAPES)
def test_numpy_optimum_at_the_feature_limit(shape, sparse):
    n, K = shape[0], shape[2]
    check_numpy_optimum(n, max_features(K), K, sparse, 0.5, [(True, True)], nlambda=4)


def test_numpy_optimum_with_a_standardized_response_and_user_lambdas():
    check_numpy_optimum(65, 13, 5, False, 0.5, [(True, True)], standardize_response=True, seed=1)
    x, y = tm.problem(65, 13, 5, False, seed=2)
    a0, beta, _ = tm.numpy_block_cd_path(x, y, tm.NONMONOTONE, 0.5)
    tm.assert_optimal(tm.numpy_kkt(a0, beta, x, y, tm.NONMONOTONE, 0.5, True, True), np.array(tm.NONMONOTONE), "user lambdas")


def test_the_certificate_sees_a_wrong_block_update():
    """The negative control of the certificate itself: coefficients 1 % off the optimum are seen (ratio > 1e-3)."""
    x, y = tm.problem(65, 13, 5, False)
    lam = automatic_lambdas(x, y, 0.5, True, 5, 1e-2)
    a0, beta, _ = tm.numpy_block_cd_path(x, y, lam, 0.5)
    k = tm.numpy_kkt(a0, beta * 1.01, x, y, lam, 0.5, True, True)
    assert k["ratio"][1:].min() > 1e-3


@pytest.mark.parametrize("case", tm.ORACLE_CASES)
def test_oracle_distance_from_its_optimum(oracle, case):
    """Where ORACLE_REL_CHANGE / ORACLE_A0_CHANGE of test_gpu_mcovariance.py come from: the oracle's own coefficients
    (intercepts) move by this much between thresh and thresh / 100.  The numpy optimum is within 10 x that of the
    oracle's, as the GPU fit has to be."""
    mix, standardize_response = case
    x, y = tm.oracle_problem()
    kw = dict(family="mgaussian", alpha=mix, standardize_response=standardize_response, maxit=100000, seed=1, **tm.ORACLE_PATH)
    ref = oracle.fit(x, y, thresh=tm.ORACLE_THRESH, **kw)
    tight = oracle.fit(x, y, thresh=tm.ORACLE_THRESH / 100, **kw)
    assert (ref["return_codes"] == 0).all() and (tight["return_codes"] == 0).all()
    scale, a0_scale = np.abs(tight["beta"]).max(), max(1.0, np.abs(tight["a0"]).max())
    change = np.abs(ref["beta"] - tight["beta"]).max() / scale
    a0_change = np.abs(ref["a0"][:, 1:] - tight["a0"][:, 1:]).max() / a0_scale
    print("oracle, mix %g standardize_response %d: change between thresh %g and thresh / 100: coefficients %.3g of max|beta|, "
          "intercepts %.3g" % (mix, standardize_response, tm.ORACLE_THRESH, change, a0_change))
    assert change <= tm.ORACLE_REL_CHANGE[case] and a0_change <= tm.ORACLE_A0_CHANGE[case]
    a0, beta, dev = tm.numpy_block_cd_path(x, y, ref["lambda"], mix, standardize_response=standardize_response)
    err = np.abs(beta - ref["beta"]).max() / scale
    a0_err = np.abs(a0[:, 1:] - ref["a0"][:, 1:]).max() / a0_scale
    print("numpy optimum vs oracle: coefficients %.3g intercepts %.3g dev_ratio %.3g" % (err, a0_err, np.abs(dev[1:] - ref["dev_ratio"][1:]).max()))
    assert err <= 10 * tm.ORACLE_REL_CHANGE[case] and a0_err <= 10 * tm.ORACLE_A0_CHANGE[case]
    assert np.abs(dev[1:] - ref["dev_ratio"][1:]).max() <= 10 * tm.ORACLE_REL_CHANGE[case]


def test_oracle_has_no_optimum_with_a_ridge_part(oracle):
    """The negative control: at mix = 0.5 the reference iteration (the oracle; every SAGA mode follows it) stops far from
    the optimum of the stated problem, which is why the new mode has no oracle to be compared with there."""
    x, y = tm.oracle_problem()
    ref = oracle.fit(x, y, family="mgaussian", alpha=0.5, thresh=tm.ORACLE_THRESH, maxit=5000, seed=1, **tm.ORACLE_PATH)
    k = tm.numpy_kkt(ref["a0"], ref["beta"], x, y, ref["lambda"], 0.5, True, True)
    print("oracle at mix 0.5: KKT ratio per lambda", k["ratio"], "return codes", ref["return_codes"])
    assert k["ratio"][1:].max() > 1e-3
    a0, beta, _ = tm.numpy_block_cd_path(x, y, ref["lambda"], 0.5)
    tm.assert_optimal(tm.numpy_kkt(a0, beta, x, y, ref["lambda"], 0.5, True, True), ref["lambda"], "numpy at mix 0.5")
