"""SGDNET_MODE_WNEWTON on the CPU: the header, the binding, the package and the shim agree; the feature limit is the LDS
budget written in csrc/newton.hpp; and the algorithm restated in numpy (tests/wnewton_reference.py) reaches the project's
optimality bound on every input tests/test_gpu_wnewton.py gives the device, with every return code 0, and agrees with
newton mode's restatement where that mode runs -- so the bounds ask nothing of the device that the method and f64 do not
give."""
import os
import re

import numpy as np
import pytest

import test_gpu_newton as tn
import wnewton_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the two restatements on the same input: the same optimum to this fraction of max|beta| (measured: 3.2e-15 at most; both
# stop at thresh = 1e-12, so their last steps may differ by that much)
RESTATEMENTS_REL = 1e-11


def test_header_binding_package_and_shim_agree():
    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sgdnet_hip.h")).read()
    assert int(re.search(r"#define SGDNET_MODE_WNEWTON\s+(\d+)", hdr).group(1)) == _lib.MODE_WNEWTON == 8
    assert int(re.search(r"#define SGDNET_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 6
    assert re.search(r"int sgdnet_wnewton_max_features\(void\);", hdr) and '"wnewton_width"' in hdr
    assert "sgdnet_wnewton_max_features" in _lib.EXPORTS
    assert "sgdnet_wnewton" in sa.__all__ and "wnewton_max_features" in sa.__all__
    assert _lib.MODES == {"exact": 0, "batched": 1, "auto": 2, "covariance": 3}      # sgdnet(mode=...) does not reach mode 8
    shim = open(os.path.join(ROOT, "shim", "sgdnet_shim.c")).read()
    assert '"wnewton") == 0) c->mode = SGDNET_MODE_WNEWTON' in shim
    # (what the plan refuses of this mode, rung by rung and byte for byte: test_direct_plan_host.py)


def test_feature_limit_is_the_lds_budget():
    # (newton.hpp's wnewton_state_bytes is wr.state_bytes, value by value: test_direct_plan_host.py)
    p = wr.LIMIT
    assert p == 5819 and p >= 4096
    assert wr.state_bytes(p + 1) <= wr.LDS_BYTES < wr.state_bytes(p + 2)
    try:
        import sgdnet_amd as sa
        assert sa.wnewton_max_features() == p
    except OSError:
        pass                                                    # (the library does not load here: the compiled header is the check)


def test_mode_string_is_not_one_of_sgdnet():
    import sgdnet_amd as sa
    x = np.random.default_rng(0).standard_normal((20, 3))
    y = (x[:, 0] > 0).astype(float)
    with pytest.raises(ValueError, match="mode must be one of"):
        sa.sgdnet(x, y, family="binomial", nlambda=3, mode="wnewton")
    if sa.load().sgdnet_device_count() == 0:
        # sgdnet_wnewton passes the argument mapping and reaches the backend, which has no device to run on
        with pytest.raises(sa.SgdnetError) as e:
            sa.sgdnet_wnewton(x, y, nlambda=3)
        assert e.value.code == -2


def test_width_option_is_one_of_the_library():
    import sgdnet_amd as sa
    assert sa.get_option("wnewton_width") == 0
    with sa.option("wnewton_width", 1024):
        assert sa.get_option("wnewton_width") == 1024
    with pytest.raises(sa.SgdnetError):
        sa.set_option("wnewton_width", 2048)
    assert sa.get_option("wnewton_width") == 0


def check_restatement(x, y, lam, mix, standardize, intercept, what, newton_too=False):
    a0, beta, info = wr.numpy_wide_newton_path(x, y, lam, mix, standardize, intercept)
    print(what, "outer steps", info["steps"], "most screens of a solve", info["screens"], "most list sweeps", info["sweeps"])
    assert info["codes"] == [0] * len(lam), (what, info["codes"])
    tn.assert_optimal(tn.numpy_kkt(a0, beta, x, y, lam, mix, standardize, intercept), np.asarray(lam, dtype=float), what)
    if newton_too:
        b0, bb, binfo = tn.numpy_newton_path(x, y, lam, mix, standardize, intercept)
        scale = max(np.abs(bb).max(), 1e-300)
        diff = max(np.abs(beta - bb).max(), np.abs(a0 - b0).max()) / scale
        print(what, "against newton mode's restatement: %.3g of max|beta|; state passes %d against %d" % (diff, info["passes"], binfo["passes"]))
        assert diff <= RESTATEMENTS_REL, (what, diff)
        return info, binfo
    return info, None


@pytest.mark.parametrize("mix", wr.MIXES)
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", wr.SHAPES)
def test_restatement_is_optimal_on_the_gpu_inputs(shape, sparse, mix):
    """test_gpu_wnewton.py::test_automatic_path_is_optimal, input by input; where newton mode takes the shape, its
    restatement gives the same optimum"""
    n, p = shape[0], shape[1] or wr.LIMIT
    x, y = tn.problem(n, p, sparse)
    nlambda, ratio = wr.path_of(shape[0], shape[1], mix)
    for intercept, standardize in wr.settings_of(shape[1]):
        lam = wr.automatic_lambdas(x, y, mix, standardize, nlambda, ratio)
        check_restatement(x, y, lam, mix, standardize, intercept, (n, p, sparse, mix, intercept, standardize), newton_too=p <= 198)


@pytest.mark.parametrize("shape", wr.WIDTH_SHAPES)
def test_restatement_is_optimal_on_the_width_inputs(shape):
    """test_gpu_wnewton.py::test_both_widths_and_a_second_call_give_the_same_bits: its further dense inputs, on its path"""
    x, y = tn.problem(shape[0], shape[1], False)
    nlambda, ratio = wr.path_of(shape[0], shape[1], 0.5)
    lam = wr.automatic_lambdas(x, y, 0.5, True, nlambda, ratio)
    check_restatement(x, y, lam, 0.5, True, True, ("width", shape), newton_too=shape[1] <= 198)


@pytest.mark.parametrize("sparse", [False, True])
def test_restatements_agree_where_both_modes_run(sparse):
    """test_gpu_wnewton.py::test_same_optimum_as_newton_mode_in_as_many_passes: the optimum, and the passes the curvature
    guard allows -- the wide restatement takes no more state passes than newton mode's on any of these inputs"""
    for n, p in wr.BOTH_MODES:
        x, y = tn.problem(n, p, sparse, seed=3)
        for mix in (0.5, 0.0):
            lam = wr.automatic_lambdas(x, y, mix, True, wr.BOTH_MODES_PATH["nlambda"], wr.BOTH_MODES_PATH["lambda_min_ratio"])
            info, binfo = check_restatement(x, y, lam, mix, True, True, ("both modes", n, p, sparse, mix), newton_too=True)
            assert info["passes"] - binfo["passes"] <= 0          # test_gpu_wnewton.py: RESTATEMENT_EXCESS_PASSES


@pytest.mark.parametrize("sparse", [False, True])
def test_restatement_on_the_other_gpu_inputs(sparse):
    """the column of mean 1e6 and its centred twin, the user's lambdas, and maxit = 2"""
    shifted, centred, y = wr.large_mean_twins(sparse)
    lam = wr.automatic_lambdas(centred, y, wr.LARGE_MEAN["alpha"], True, wr.LARGE_MEAN["nlambda"], wr.LARGE_MEAN["lambda_min_ratio"])
    check_restatement(centred, y, lam, 0.5, True, True, ("centred twin", sparse), newton_too=True)
    a0, beta, info = wr.numpy_wide_newton_path(shifted, y, lam, 0.5)
    b0, bb, _ = wr.numpy_wide_newton_path(centred, y, lam, 0.5)
    assert info["codes"] == [0] * len(lam) and np.abs(beta - bb).max() <= wr.LARGE_MEAN_TOL * np.abs(bb).max()
    x, y = tn.problem(300, 199, sparse, seed=1)
    check_restatement(x, y, tn.NONMONOTONE, 0.5, True, True, ("user lambdas", sparse))
    if not sparse:
        x, y = tn.problem(300, 199, False, seed=2)
        lam = wr.automatic_lambdas(x, y, 0.5, True, 5, 1e-2)
        _, _, short = wr.numpy_wide_newton_path(x, y, lam, 0.5, thresh=1e-14, maxit=2)
        _, _, full = wr.numpy_wide_newton_path(x, y, lam, 0.5, thresh=1e-14)
        assert short["codes"][1:] == [1] * 4 and min(full["steps"][1:]) >= 5 and full["codes"] == [0] * 5


def test_rescreen_input_sends_a_converged_list_back_to_the_screen():
    """In some inner solve the list converges, the next screen adds to it, and only a later one adds nothing: three
    screens at least (two is the minimum of every solve)."""
    x, y = wr.rescreen_problem()
    lam = wr.automatic_lambdas(x, y, wr.RESCREEN["alpha"], True, wr.RESCREEN["nlambda"], wr.RESCREEN["lambda_min_ratio"])
    info, _ = check_restatement(x, y, lam, wr.RESCREEN["alpha"], True, True, "re-screen")
    assert min(info["screens"]) >= 2 and max(info["screens"]) >= 3, info["screens"]
    assert max(info["sweeps"]) < wr.MAX_SWEEPS                   # (no solve of this input is cut short)
