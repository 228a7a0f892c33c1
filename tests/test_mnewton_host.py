"""sa.sgdnet_mnewton without a GPU: the constants of the three layers, the LDS budget, and the numpy restatement of the
algorithm (tests/test_gpu_mnewton.py: numpy_mnewton_path) that the GPU tests' inputs and bounds lean on.

Measured (plain f64, thresh = 1e-12): the worst KKT ratio of the restatement's optimum over every input of the GPU tests
is 9.3e-10 (iris without intercept and standardisation at mix = 1: the unscaled columns make the inner solve's relative
stopping rule loosest there), the worst intercept residual 1.7e-11 lambda, and the dev_ratio from the state pass is within
3.7e-15 of the returned coefficients'; the bounds
asked of the device are 1e-8 and 1e-10.  The oracle's distances are in test_gpu_mnewton.py (ORACLE_*); at its default
thresh the oracle's iris path is up to 1.4e-2 lambda from its optimum (test_oracle_at_the_default_thresh_is_far)."""
import os
import re

import numpy as np
import pytest

import test_gpu_mnewton as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_DOUBLES = 160 * 1024 // 8
LIMITS = {2: 98, 3: 65, 4: 48, 5: 38, 10: 18, 99: 1}


def state_doubles(Q):
    return Q * (Q + 1) // 2 + 2 * Q


def max_features(K):
    """sgdnet_mnewton_max_features: through the library where it loads, else restated from mnewton.hpp's text."""
    try:
        import sgdnet_amd as sa
        return sa.mnewton_max_features(K)
    except OSError:
        # (mnewton.hpp's mnewton_max_features at the K of LIMITS, from the compiled header: test_direct_plan_host.py)
        Q = 1
        while state_doubles(Q + 1) <= LDS_DOUBLES:
            Q += 1
        return max(Q // K - 1, 0) if 2 <= K <= Q else 0


def test_header_binding_package_and_shim_agree():
    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sgdnet_hip.h")).read()
    assert int(re.search(r"#define SGDNET_MODE_MNEWTON\s+(\d+)", hdr).group(1)) == _lib.MODE_MNEWTON == 6
    assert int(re.search(r"#define SGDNET_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 6
    assert re.search(r"int sgdnet_mnewton_max_features\(int n_classes\);", hdr)
    assert "sgdnet_mnewton_max_features" in _lib.EXPORTS
    assert "sgdnet_mnewton" in sa.__all__ and "mnewton_max_features" in sa.__all__
    assert _lib.MODES == {"exact": 0, "batched": 1, "auto": 2, "covariance": 3}      # sgdnet(mode=...) does not reach mode 6
    shim = open(os.path.join(ROOT, "shim", "sgdnet_shim.c")).read()
    assert '"mnewton") == 0) c->mode = SGDNET_MODE_MNEWTON' in shim
    # (what the plan refuses of this mode, rung by rung and byte for byte: test_direct_plan_host.py)
    assert "mnewton.hip" in open(os.path.join(ROOT, "build.sh")).read()
    # the restated constants are newton.hpp's, which mnewton.hip takes as they are
    nwt = open(os.path.join(ROOT, "sgdnet_amd", "csrc", "newton.hpp")).read()
    assert "kNewtonMaxHalvings = %d;" % tm.MAX_HALVINGS in nwt and "kNewtonMaxSweeps = %d;" % tm.MAX_SWEEPS in nwt
    assert "kNewtonObjectiveSlack = 1e-12;" in nwt and "kNewtonNegligible = 16 * 2.220446049250313e-16;" in nwt
    src = open(os.path.join(ROOT, "sgdnet_amd", "csrc", "mnewton.hip")).read()
    for name in ("kNewtonMaxHalvings", "kNewtonObjectiveSlack", "kNewtonNegligible", "kNewtonMaxSweeps"):
        assert name in src and not re.search(r"constexpr[^;]*\b%s\b" % name, src)


def test_mode_string_is_not_one_of_sgdnet():
    import sgdnet_amd as sa
    x, y = tm.iris()
    with pytest.raises(ValueError, match="mode must be one of"):
        sa.sgdnet(x, y, family="multinomial", nlambda=3, mode="mnewton")
    if sa.load().sgdnet_device_count() == 0:
        # sgdnet_mnewton passes the argument mapping and reaches the backend, which has no device to run on
        with pytest.raises(sa.SgdnetError) as e:
            sa.sgdnet_mnewton(x, y, nlambda=3)
        assert e.value.code == -2


@pytest.mark.parametrize("K", sorted(LIMITS))
def test_feature_limit_is_the_lds_budget(K):
    assert max_features(K) == LIMITS[K] == 199 // K - 1


def test_feature_limit_where_nothing_fits():
    for K in (-3, 0, 1, 100, 101, 199, 200, 2 ** 31 - 1):
        assert max_features(K) == 0


@pytest.mark.parametrize("K", [2, 3, 10])
def test_lds_arithmetic_at_the_limit(K):
    p = max_features(K)
    assert state_doubles(K * (p + 1)) <= LDS_DOUBLES                     # the limit fits
    # one more feature: past the 199 coordinates, of which 200 no longer fit
    assert K * (p + 2) > 199 and state_doubles(199) <= LDS_DOUBLES < state_doubles(200)
    assert state_doubles(199) == 19900 + 398


def check_numpy_optimum(x, y, K, mix, settings, nlambda, ratio, what):
    for intercept, standardize in settings:
        lam = tm.automatic_lambdas(x, y, K, mix, standardize, nlambda, ratio)
        a0, beta, dev, info = tm.numpy_mnewton_path(x, y, K, lam, mix, standardize, intercept)
        assert info["codes"] == [0] * nlambda
        k = tm.numpy_kkt(a0, beta, x, y, lam, mix, standardize, intercept)
        tm.assert_optimal(k, lam, (what, mix, intercept, standardize))
        ref = tm.numpy_dev_ratio(a0, beta, x, y, standardize, intercept)
        print("state pass vs coefficients: dev_ratio differs by %.3g; steps %s sweeps %d halvings %d"
              % (np.abs(dev - ref).max(), info["steps"], info["sweeps"], info["halvings"]))
        assert np.abs(dev - ref).max() <= tm.DEV_TOL


@pytest.mark.parametrize("mix", tm.MIXES)
def test_numpy_optimum_on_iris_is_inside_the_bound(mix):
    x, y = tm.iris()
    check_numpy_optimum(x, y, 3, mix, tm.SETTINGS, 6, 1e-2, "iris")


@pytest.mark.parametrize("mix", tm.MIXES)
@pytest.mark.parametrize("shape", tm.TILE_SHAPES + tm.ROW_SHAPES + tm.CLASS_SHAPES)
def test_numpy_optimum_is_inside_the_bound(shape, mix):
    """The inputs of test_gpu_mnewton.py::test_automatic_path_is_optimal: an optimum computed in plain f64 passes the same
    checks, so the bounds ask nothing of the device that the number format does not give."""
    x, y = tm.problem(*shape)
    check_numpy_optimum(x, y, shape[2], mix, tm.SETTINGS, tm.NLAMBDA, tm.ratio_for(shape), shape)


@pytest.mark.parametrize("shape", tm.LIMIT_SHAPES)
def test_numpy_optimum_at_the_feature_limit(shape):
    n, K = shape[0], shape[2]
    x, y = tm.problem(n, max_features(K), K)
    check_numpy_optimum(x, y, K, 0.5, [(True, True)], 4, tm.ratio_for(shape), shape)


def test_numpy_optimum_of_the_other_inputs():
    x, y = tm.problem(200, 6, 5, seed=2)
    a0, beta, _, _ = tm.numpy_mnewton_path(x, y, 5, tm.NONMONOTONE, 0.5)
    tm.assert_optimal(tm.numpy_kkt(a0, beta, x, y, tm.NONMONOTONE, 0.5, True, True), np.array(tm.NONMONOTONE), "user lambdas")
    x, y = tm.problem(160, 5, 4, seed=5)
    x[:, 2] = 3.0
    check_numpy_optimum(x, y, 4, 1.0, [(True, True), (True, False)], 5, 1e-2, "constant column")
    x, y = tm.problem(120, 4, 3, seed=6)
    y[y == 2] = 1.0
    y[7] = 2.0
    check_numpy_optimum(x, y, 3, 0.5, [(True, True)], 5, 1e-2, "single member")


def test_numpy_path_starts_with_exact_zeros():
    """At lambda_max the threshold's rounding residue is snapped to 0.0 (kNewtonNegligible): what
    test_gpu_mnewton.py::test_lambda_max_first asks of the device."""
    x, y = tm.iris()
    for intercept, standardize in tm.SETTINGS:
        for mix in (1.0, 0.5):
            lam = tm.automatic_lambdas(x, y, 3, mix, standardize, 4, 1e-4)
            _, beta, _, info = tm.numpy_mnewton_path(x, y, 3, lam, mix, standardize, intercept)
            assert (beta[:, :, 0] == 0.0).all() and info["codes"][0] == 0, (intercept, standardize, mix, beta[:, :, 0])
    x, y = tm.problem(200, 6, 5)
    lam = tm.automatic_lambdas(x, y, 5, 1.0, True, 4, 1e-4)
    assert (tm.numpy_mnewton_path(x, y, 5, lam, 1.0)[1][:, :, 0] == 0.0).all()


def test_the_certificate_sees_a_wrong_step():
    """The negative control of the certificate itself: coefficients 1 % off the optimum are seen (ratio > 1e-3)."""
    x, y = tm.iris()
    lam = tm.automatic_lambdas(x, y, 3, 0.5, True, 5, 1e-2)
    a0, beta, _, _ = tm.numpy_mnewton_path(x, y, 3, lam, 0.5)
    assert tm.numpy_kkt(a0, beta * 1.01, x, y, lam, 0.5, True, True)["ratio"][1:].min() > 1e-3


@pytest.mark.parametrize("mix", tm.ORACLE_MIXES)
def test_oracle_distance_from_the_optimum_on_iris(oracle, mix):
    """Where ORACLE_*_DIST of test_gpu_mnewton.py come from: the oracle at ORACLE_THRESH against the restatement's
    optimum (itself within 1e-11 lambda of stationarity, see above), from the second lambda on for intercepts and deviances:
    at lambda_max the oracle's stopping rule (coefficients only, all zero) leaves ITS intercepts short."""
    x, y = tm.iris()
    ref = oracle.fit(x, y, family="multinomial", n_classes=3, alpha=mix, thresh=tm.ORACLE_THRESH, maxit=100000, seed=1, **tm.ORACLE_PATH)
    assert (ref["return_codes"] == 0).all()
    a0, beta, dev, _ = tm.numpy_mnewton_path(x, y, 3, ref["lambda"], mix)
    ra = tm.centred(ref["a0"])
    err = np.abs(beta - ref["beta"]).max() / np.abs(ref["beta"]).max()
    a0_err = np.abs(a0[:, 1:] - ra[:, 1:]).max() / max(1.0, np.abs(ra).max())
    dev_err = np.abs(dev[1:] - ref["dev_ratio"][1:]).max()
    print("oracle at thresh %g, mix %g: coefficients %.3g of max|beta|, intercepts %.3g, dev_ratio %.3g" % (tm.ORACLE_THRESH, mix, err, a0_err, dev_err))
    assert err <= tm.ORACLE_BETA_DIST[mix] and a0_err <= tm.ORACLE_A0_DIST[mix] and dev_err <= tm.ORACLE_DEV_DIST[mix]


def test_oracle_at_the_default_thresh_is_far(oracle):
    """The negative control: at the default thresh the oracle's iris path (every SAGA mode follows it) is far outside the
    bound the new mode is held to -- measured 1.5e-4 lambda at the second lambda, 1.4e-2 lambda at the last."""
    x, y = tm.iris()
    ref = oracle.fit(x, y, family="multinomial", n_classes=3, alpha=0.5, seed=1, **tm.ORACLE_PATH)
    k = tm.numpy_kkt(tm.centred(ref["a0"]), ref["beta"], x, y, ref["lambda"], 0.5, True, True)
    print("oracle at the default thresh: KKT ratio per lambda", k["ratio"])
    assert k["ratio"][1:].min() > 1e3 * tm.KKT_BOUND
