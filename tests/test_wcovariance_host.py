"""SGDNET_MODE_WCOVARIANCE on the CPU: the header, the binding, the package and the shim agree; the feature limit is the
LDS budget written in csrc/covariance.hpp; and the algorithm restated in numpy (tests/wcovariance_reference.py) reaches
the project's optimality bound on every input tests/test_gpu_wcovariance.py gives the device, in fewer list sweeps per
lambda than the maxit that test passes -- so the bound and the sweep limit ask nothing of the device that the method and
f64 do not give."""
import os
import re

import numpy as np
import pytest

import test_gpu_covariance as tc
import wcovariance_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_BYTES = 160 * 1024


def state_bytes(p):
    """4 p doubles, p list words, one bit per coordinate in whole words, the compaction's 2 x 16 counts"""
    return 32 * p + 4 * p + 4 * ((p + 31) // 32) + 4 * 2 * 16


def max_features():
    """sgdnet_wcovariance_max_features: through the library where it loads, else restated from covariance.hpp's budget."""
    try:
        import sgdnet_amd as sa
        return sa.wcovariance_max_features()
    except OSError:
        p = 1
        while state_bytes(p + 1) <= LDS_BYTES:
            p += 1
        return p


def test_header_binding_package_and_shim_agree():
    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sgdnet_hip.h")).read()
    assert int(re.search(r"#define SGDNET_MODE_WCOVARIANCE\s+(\d+)", hdr).group(1)) == _lib.MODE_WCOVARIANCE == 7
    assert int(re.search(r"#define SGDNET_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 6
    assert re.search(r"int sgdnet_wcovariance_max_features\(void\);", hdr)
    assert "sgdnet_wcovariance_max_features" in _lib.EXPORTS
    assert "sgdnet_wcovariance" in sa.__all__ and "wcovariance_max_features" in sa.__all__
    assert _lib.MODES == {"exact": 0, "batched": 1, "auto": 2, "covariance": 3}      # sgdnet(mode=...) does not reach mode 7
    shim = open(os.path.join(ROOT, "shim", "sgdnet_shim.c")).read()
    assert '"wcovariance") == 0) c->mode = SGDNET_MODE_WCOVARIANCE' in shim
    # (what the plan refuses of this mode, rung by rung and byte for byte: test_direct_plan_host.py)


def test_feature_limit_is_the_lds_budget():
    # (covariance.hpp's wcov_state_bytes is state_bytes above, value by value: test_direct_plan_host.py)
    p = max_features()
    assert p == wr.LIMIT and p >= 4096
    assert state_bytes(p) <= LDS_BYTES < state_bytes(p + 1)


def test_mode_string_is_not_one_of_sgdnet():
    import sgdnet_amd as sa
    x = np.random.default_rng(0).standard_normal((20, 3))
    y = x[:, 0] + 1.0
    with pytest.raises(ValueError, match="mode must be one of"):
        sa.sgdnet(x, y, nlambda=3, mode="wcovariance")
    if sa.load().sgdnet_device_count() == 0:
        # sgdnet_wcovariance passes the argument mapping and reaches the backend, which has no device to run on
        with pytest.raises(sa.SgdnetError) as e:
            sa.sgdnet_wcovariance(x, y, nlambda=3)
        assert e.value.code == -2


def test_width_option_is_one_of_the_library():
    import sgdnet_amd as sa
    assert sa.get_option("wcovariance_width") == 0
    with sa.option("wcovariance_width", 1024):
        assert sa.get_option("wcovariance_width") == 1024
    with pytest.raises(sa.SgdnetError):
        sa.set_option("wcovariance_width", 2048)
    assert sa.get_option("wcovariance_width") == 0


def check_restatement(x, y, lam, mix, standardize, intercept, what):
    a0, beta, sweeps, screens, unconverged = wr.numpy_wide_path(x, y, lam, mix, standardize, intercept)
    print(what, "most list sweeps per lambda %d, most screens %d" % (sweeps.max(), screens.max()))
    assert not unconverged.any() and sweeps.max() < wr.MAXIT, (what, sweeps)
    tc.assert_optimal(tc.numpy_kkt(a0, beta, x, y, lam, mix, standardize, intercept), np.asarray(lam, dtype=float), what)
    return sweeps, screens


@pytest.mark.parametrize("mix", wr.MIXES)
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", wr.SHAPES)
def test_restatement_is_optimal_on_the_gpu_inputs(shape, sparse, mix):
    """test_gpu_wcovariance.py::test_automatic_path_is_optimal, input by input"""
    n, p = shape[0], shape[1] or wr.LIMIT
    x, y = tc.problem(n, p, sparse)
    nlambda, ratio = wr.path_of(shape[0], shape[1], mix)
    for intercept, standardize in wr.settings_of(shape[1]):
        lam = wr.automatic_lambdas(x, y, mix, standardize, nlambda, ratio)
        check_restatement(x, y, lam, mix, standardize, intercept, (n, p, sparse, mix, intercept, standardize))


@pytest.mark.parametrize("shape", wr.WIDTH_SHAPES)
def test_restatement_is_optimal_on_the_width_inputs(shape):
    """test_gpu_wcovariance.py::test_both_widths_and_a_second_call_give_the_same_bits: its further dense inputs, on its path"""
    x, y = tc.problem(shape[0], shape[1], False)
    lam = wr.automatic_lambdas(x, y, 0.5, True, wr.WIDTH_PATH["nlambda"], wr.WIDTH_PATH["lambda_min_ratio"])
    check_restatement(x, y, lam, 0.5, True, True, ("width", shape))


@pytest.mark.parametrize("sparse", [False, True])
def test_restatement_on_the_other_gpu_inputs(sparse):
    """the column of mean 1e6, the inputs shared with mode = covariance and the user's lambdas"""
    x, y = wr.large_mean_problem(sparse)
    check_restatement(x, y, wr.automatic_lambdas(x, y, 0.5, True, 6, 1e-2), 0.5, True, True, ("mean 1e6", sparse))
    for n, p in ((600, 198), (200, 33)):
        x, y = tc.problem(n, p, sparse, seed=3)
        for mix in (0.5, 0.0):
            check_restatement(x, y, wr.automatic_lambdas(x, y, mix, True, 6, 1e-2), mix, True, True, ("both modes", n, p, sparse, mix))
    x, y = tc.problem(300, 199, sparse, seed=1)
    check_restatement(x, y, tc.NONMONOTONE, 0.5, True, True, ("user lambdas", sparse))


def test_rescreen_input_sends_the_algorithm_back_to_the_screen():
    """At some lambda the list converges, the next screen adds to it, and only a later one adds nothing: three screens
    at least (two is the minimum of every lambda)."""
    x, y = wr.rescreen_problem()
    lam = wr.automatic_lambdas(x, y, wr.RESCREEN["alpha"], True, wr.RESCREEN["nlambda"], wr.RESCREEN["lambda_min_ratio"])
    sweeps, screens = check_restatement(x, y, lam, wr.RESCREEN["alpha"], True, True, "re-screen")
    assert screens.min() >= 2 and screens.max() >= 3, screens
