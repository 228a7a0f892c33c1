"""SGDNET_MODE_WMNEWTON on the CPU: the header, the binding, the package and the shim agree; the feature limit, the LDS
budget and the row chunks are those written in csrc/mnewton.hpp (a stand-alone host program built with g++ from
fit_plan.hpp prints them); the plan refuses what it must, rung by rung, with the text plan_direct's template gives; and
the algorithm restated in numpy (tests/wmnewton_reference.py) reaches the project's optimality bound on every input
tests/test_gpu_wmnewton.py gives the device, with every return code 0, and agrees with mnewton mode's restatement where
that mode runs -- so the bounds ask nothing of the device that the method and f64 do not give."""
import os
import re

import numpy as np
import pytest

import test_direct_plan_host as dp
import test_gpu_mnewton as tm
import wmnewton_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE = 10
GAUSSIAN, BINOMIAL, MULTINOMIAL, MGAUSSIAN = dp.GAUSSIAN, dp.BINOMIAL, dp.MULTINOMIAL, dp.MGAUSSIAN
# The two restatements on the same input, where both modes run -- the bounds tests/test_gpu_wmnewton.py asks of the device
# (tests/test_gpu_wnewton.py's figures): coefficients and intercepts relative to max|beta|, dev_ratio absolute, and the
# total state passes of the wide mode less mnewton mode's.
# Measured over BOTH_MODES x mixes (dense, the default setting): coefficients 4.9e-15 at most where they are unique (1.5e-2
# at (160, 5, 4), mix 1: the even K of DESIGN.md 4.6), intercepts 4.0e-15, dev_ratio 2.2e-16, excess passes 0 everywhere.
SAME_OPTIMUM_REL, SAME_DEV_RATIO, EXCESS_PASSES = 1e-9, 1e-10, 0


# ---- the three layers ----

def test_header_binding_package_and_shim_agree():
    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sgdnet_hip.h")).read()
    assert int(re.search(r"#define SGDNET_MODE_WMNEWTON\s+(\d+)", hdr).group(1)) == _lib.MODE_WMNEWTON == MODE
    assert int(re.search(r"#define SGDNET_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 6
    assert re.search(r"int sgdnet_wmnewton_max_features\(int n_classes\);", hdr) and '"wmnewton_width"' in hdr
    assert "sgdnet_wmnewton_max_features" in _lib.EXPORTS
    assert "sgdnet_wmnewton" in sa.__all__ and "wmnewton_max_features" in sa.__all__
    assert _lib.MODES == {"exact": 0, "batched": 1, "auto": 2, "covariance": 3}      # sgdnet(mode=...) does not reach mode 10
    shim = open(os.path.join(ROOT, "shim", "sgdnet_shim.c")).read()
    assert '"wmnewton") == 0) c->mode = SGDNET_MODE_WMNEWTON' in shim
    # the restated constants are newton.hpp's, which mnewton.hip takes as they are
    src = open(os.path.join(ROOT, "sgdnet_amd", "csrc", "mnewton.hip")).read()
    for name in ("mnewton_wide_scale_kernel", "mnewton_wide_cd_kernel", "mnewton_wide_blend_kernel", "mnewton_coord_new_u"):
        assert name in src


def test_mode_string_is_not_one_of_sgdnet():
    import sgdnet_amd as sa
    x, y = tm.iris()
    with pytest.raises(ValueError, match="mode must be one of"):
        sa.sgdnet(x, y, family="multinomial", nlambda=3, mode="wmnewton")
    if sa.load().sgdnet_device_count() == 0:
        # sgdnet_wmnewton passes the argument mapping and reaches the backend, which has no device to run on
        with pytest.raises(sa.SgdnetError) as e:
            sa.sgdnet_wmnewton(x, y, nlambda=3)
        assert e.value.code == -2


def test_width_option_is_one_of_the_library():
    import sgdnet_amd as sa
    assert sa.get_option("wmnewton_width") == 0
    with sa.option("wmnewton_width", 1024):
        assert sa.get_option("wmnewton_width") == 1024
    with pytest.raises(sa.SgdnetError):
        sa.set_option("wmnewton_width", 2048)
    assert sa.get_option("wmnewton_width") == 0


def test_limit_through_the_library_is_the_restated_one():
    import sgdnet_amd as sa
    assert [sa.wmnewton_max_features(K) for K in wr.LIMIT_KS] == [wr.max_features(K) for K in wr.LIMIT_KS]


# ---- the compiled header: budget, limit, chunks ----

CHUNK_N = [1, 40, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 5000, 100000, 262144, 262145, 10000000]
CHUNK_P = [1, 2, 13, 14, 15, 30, 57, 100, 340, 500, 581, 2909]
CHUNK_K = [2, 3, 10, 99]

BUDGETS = '''#include "fit_plan.hpp"
#include <cstdio>
using namespace sgdnet;
int main() {
  const int Ks[] = {%s};
  for (int K : Ks) printf("%%d ", wmnewton_max_features(K));
  printf("\\n");
  for (int Q = 1; Q <= 5822; ++Q) printf("%%d\\n", wmnewton_state_bytes(Q));
  const long long ns[] = {%s}, ps[] = {%s}, Kc[] = {%s};
  for (long long n : ns) for (long long p : ps) for (long long K : Kc)
    printf("%%lld %%lld\\n", (long long)wmnewton_row_chunks(n, p + 2, K), (long long)wmnewton_rows_per_chunk(n, p + 2, K, %d));
  for (int m = 0; m <= 11; ++m) printf("%%d", plans_direct(m) ? 1 : 0);
  printf("\\n%%d %%d\\n", kWmnewtonMaxCoordinates, kWmnewtonLdsBytes);
  return 0;
}
'''


def join(values):
    return ", ".join(str(v) for v in values)


def test_budget_limit_and_chunks_are_the_restated_ones(tmp_path):
    text = BUDGETS % (join(wr.LIMIT_KS), join(CHUNK_N), join(CHUNK_P), join(CHUNK_K), wr.TILE_ROWS)
    out = dp.compile_and_run(str(tmp_path), "wmnewton_budgets", text).split("\n")
    limits = [int(v) for v in out[0].split()]
    assert limits == [wr.max_features(K) for K in wr.LIMIT_KS] == [0, 0, 0, 2909, 1939, 1454, 1163, 581, 290, 115, 57, 0, 0]
    for K, p in wr.LIMIT_TABLE.items():
        assert wr.max_features(K) == p == 5820 // K - 1
    for Q in range(1, 5823):
        assert int(out[Q]) == wr.state_bytes(Q), Q
    assert wr.MAX_COORDINATES == 5820 and wr.state_bytes(5820) <= wr.LDS_BYTES < wr.state_bytes(5821)
    at = 5823
    for n in CHUNK_N:
        for p in CHUNK_P:
            for K in CHUNK_K:
                assert [int(v) for v in out[at].split()] == [wr.row_chunks(n, p, K), wr.rows_per_chunk(n, p, K)], (n, p, K)
                at += 1
    assert out[at] == "000111111110"                           # plans_direct over the mode numbers 0 .. 11: 3 .. 10 and no other
    assert [int(v) for v in out[at + 1].split()] == [5820, wr.LDS_BYTES]


def test_chunk_rule_says_what_it_should():
    """about 1024 workgroups, no chunk shorter than 256 rows, one chunk once a chunk has 1024 workgroups, whole staging steps"""
    for n in CHUNK_N:
        for p in CHUNK_P:
            for K in CHUNK_K:
                wg, c, r = wr.tile_pairs(p + 2) * (K * (K + 1) // 2), wr.row_chunks(n, p, K), wr.rows_per_chunk(n, p, K)
                assert c >= 1 and c * wg <= max(wg, 1024) and (c == 1 or (c - 1) * 256 < n)
                assert (wg < 1024) or c == 1
                assert r % wr.TILE_ROWS == 0 and r * c >= n and (c == 1 or r * (c - 1) < n + wr.TILE_ROWS * c)
    assert wr.row_chunks(10**6, 3, 3) == 1024 // 6 and wr.row_chunks(257, 3, 3) == 2 and wr.row_chunks(256, 3, 3) == 1
    assert wr.row_chunks(10**9, 2909, 2) == 1 and wr.row_chunks(10**9, 57, 99) == 1


# ---- the plan: every refusal rung, dense and sparse ----

def limit_of(K):
    return wr.max_features(K)


def message(what, family, K, n, p, n_gpus=1, debug=0):
    """plan_direct's template for a rule that prints the classes and the samples (fit_plan.hpp: DirectRule::kSamples)"""
    return ("mode = wmnewton needs %s: family %d, n_classes %d, %d samples, %d features (limit %d), n_gpus %d, debug %d"
            % (what, family, K, n, p, limit_of(K), n_gpus, debug))


FAMILY = "family = multinomial"
CLASSES = "2 to 99 classes"
UNGROUPED = "the ungrouped penalty (type_multinomial = 0)"
LIMIT = "no more features than sgdnet_wmnewton_max_features(n_classes)"
ONE_GPU = "one GPU (n_gpus <= 1)"
NO_DEBUG = "debug = 0 (there are no epochs to report losses of)"
DENSE_COPY = "the dense copy of a sparse x (n_samples x n_features x 8 bytes) within 1 GiB"


def plan_cases():
    """(name, case, expected needs-text or None where the plan is accepted)"""
    out = []
    n, few = 100, 5
    for sparse in (False, True):
        tag = "sparse" if sparse else "dense"
        for other in (GAUSSIAN, BINOMIAL, MGAUSSIAN):
            out.append(("family %d/%s" % (other, tag), dp.case("wmnewton", other, 3, n, few, sparse), FAMILY))
        for K in (0, 1, 100):
            out.append(("K = %d/%s" % (K, tag), dp.case("wmnewton", MULTINOMIAL, K, n, few, sparse), CLASSES))
        out.append(("grouped/%s" % tag, dp.case("wmnewton", MULTINOMIAL, 3, n, few, sparse, type_multinomial=1), UNGROUPED))
        for K in (2, 3, 99):
            out.append(("limit + 1, K = %d/%s" % (K, tag), dp.case("wmnewton", MULTINOMIAL, K, n, limit_of(K) + 1, sparse), LIMIT))
            out.append(("accepted at the limit, K = %d/%s" % (K, tag), dp.case("wmnewton", MULTINOMIAL, K, n, limit_of(K), sparse), None))
            out.append(("accepted at one feature, K = %d/%s" % (K, tag), dp.case("wmnewton", MULTINOMIAL, K, n, 1, sparse), None))
        out.append(("n_gpus/%s" % tag, dp.case("wmnewton", MULTINOMIAL, 3, n, few, sparse, n_gpus=2), ONE_GPU))
        out.append(("debug/%s" % tag, dp.case("wmnewton", MULTINOMIAL, 3, n, few, sparse, debug=1), NO_DEBUG))
        # several rungs broken at once: the first one speaks
        out.append(("limit + n_gpus + debug/%s" % tag, dp.case("wmnewton", MULTINOMIAL, 3, n, limit_of(3) + 1, sparse, n_gpus=2, debug=1), LIMIT))
        out.append(("n_gpus + debug/%s" % tag, dp.case("wmnewton", MULTINOMIAL, 3, n, few, sparse, n_gpus=2, debug=1), ONE_GPU))
        out.append(("grouped + limit/%s" % tag, dp.case("wmnewton", MULTINOMIAL, 3, n, limit_of(3) + 1, sparse, type_multinomial=1), UNGROUPED))
        out.append(("K = 100 + grouped/%s" % tag, dp.case("wmnewton", MULTINOMIAL, 100, n, few, sparse, type_multinomial=1), CLASSES))
        out.append(("all/%s" % tag, dp.case("wmnewton", BINOMIAL, 1, n, 6000, sparse, n_gpus=2, debug=1, type_multinomial=1), FAMILY))
    # the dense copy of a sparse x: n x p x 8 bytes against 1 GiB, at K = 2's limit and at a common width
    for cols in (limit_of(2), 200):
        at_bound = (1 << 30) // 8 // cols
        out.append(("dense copy, %d columns" % cols, dp.case("wmnewton", MULTINOMIAL, 2, at_bound + 1, cols, True), DENSE_COPY))
        out.append(("dense copy + debug, %d columns" % cols, dp.case("wmnewton", MULTINOMIAL, 2, at_bound + 1, cols, True, debug=1), NO_DEBUG))
        out.append(("dense copy: dense x, %d columns" % cols, dp.case("wmnewton", MULTINOMIAL, 2, at_bound + 1, cols, False), None))
        out.append(("dense copy: at the bound, %d columns" % cols, dp.case("wmnewton", MULTINOMIAL, 2, at_bound, cols, True), None))
    assert len({name for name, _, _ in out}) == len(out)
    return out


def test_plan_refuses_rung_by_rung_and_accepts_the_rest(tmp_path):
    calls = "".join('  run("%s", %d, %d, %d, %dll, %dll, %d, %d, %d, %d);\n'
                    % (name, MODE, c["family"], c["K"], c["n"], c["p"], c["sparse"], c["n_gpus"], c["debug"], c["type_multinomial"])
                    for name, c, _ in plan_cases())
    got = dp.compile_and_run(str(tmp_path), "wmnewton_plans", dp.PROGRAM % (dp.DEVICE, calls)).split("\n")
    by_name, accepted = {}, {}
    for i, line in enumerate(got):
        if line and not line.startswith("+"):
            name, rc, msg = line.split("\t")
            by_name[name] = (int(rc), msg)
            if int(rc) == 0:
                accepted[name] = got[i + 1]
    assert len(by_name) == len(plan_cases())
    for name, c, what in plan_cases():
        rc, msg = by_name[name]
        if what is None:
            assert rc == 0 and msg == "", (name, msg)
            # the mode asked for, on control.device, all the samples in one rank
            assert accepted[name] == "+\t%d\t1 %d\t2 0 %d" % (MODE, dp.DEVICE, c["n"]), name
        else:
            assert rc == dp.EUNSUPPORTED, name
            assert msg == message(what, c["family"], c["K"], c["n"], c["p"], c["n_gpus"], c["debug"]), (name, msg)


# ---- the restatement on the inputs of the GPU tests ----

def host_settings_of(shape):
    """tests/test_gpu_wmnewton.py fits the 1024-stride shapes in all four settings; the restatement (seconds per fit there)
    takes the two that differ in everything"""
    if shape in wr.STRIDE_1024:
        return [(True, True), (False, False)]
    return wr.settings_of(shape)


def check_restatement(x, y, K, lam, mix, standardize, intercept, what):
    a0, beta, dev, info = wr.numpy_wide_mnewton_path(x, y, K, lam, mix, standardize, intercept)
    k = tm.numpy_kkt(a0, beta, x, y, lam, mix, standardize, intercept)
    print(what, "outer steps", info["steps"], "most screens of a solve", info["screens"], "most list sweeps", info["sweeps"])
    assert info["codes"] == [0] * len(lam), (what, info["codes"])
    tm.assert_optimal(k, np.asarray(lam, dtype=float), what)
    ref = tm.numpy_dev_ratio(a0, beta, x, y, standardize, intercept)
    assert np.abs(dev - ref).max() <= tm.DEV_TOL, what
    return a0, beta, dev, info


@pytest.mark.parametrize("mix", wr.MIXES)
@pytest.mark.parametrize("shape", wr.SHAPES)
def test_restatement_is_optimal_on_the_gpu_inputs(shape, mix):
    """test_gpu_wmnewton.py::test_automatic_path_is_optimal, input by input (dense: the driver expands sparse x to the
    dense copy before anything is computed, so the sparse fit is the same computation).  The limit shapes run on the
    path of path_of: 2 lambdas under ridge, 3 otherwise, as the device fits them."""
    n, p, K = shape[0], wr.features_of(shape), shape[2]
    x, y = wr.problem(n, p, K)
    nlambda, ratio = wr.path_of(shape, mix)
    for intercept, standardize in host_settings_of(shape):
        lam = wr.automatic_lambdas(x, y, K, mix, standardize, nlambda, ratio)
        check_restatement(x, y, K, lam, mix, standardize, intercept, (n, p, K, mix, intercept, standardize))


@pytest.mark.parametrize("mix", wr.MIXES)
@pytest.mark.parametrize("shape", wr.BOTH_MODES)
def test_restatements_agree_where_both_modes_run(shape, mix):
    """test_gpu_wmnewton.py::test_same_optimum_as_mnewton_mode_in_as_many_passes: the optimum, and the passes the curvature
    guard allows.  Coefficients are compared only where the optimum is unique in them (mix < 1 or an odd K: DESIGN.md 4.6)."""
    n, p, K = shape
    x, y = wr.problem(n, p, K)
    nlambda, ratio = wr.path_of(shape, mix)
    lam = wr.automatic_lambdas(x, y, K, mix, True, nlambda, ratio)
    a0, beta, dev, info = check_restatement(x, y, K, lam, mix, True, True, ("both modes", shape, mix))
    b0, bb, bdev, binfo = tm.numpy_mnewton_path(x, y, K, lam, mix)
    assert binfo["codes"] == [0] * len(lam)
    scale = max(np.abs(bb).max(), 1e-300)
    coef, icpt, ddev = np.abs(beta - bb).max() / scale, np.abs(a0 - b0).max() / scale, np.abs(dev - bdev).max()
    excess = info["passes"] - binfo["passes"]
    print(shape, mix, "wide against mnewton's restatement: coefficients %.3g intercepts %.3g of max|beta|, dev_ratio %.3g, state passes %d "
          "against %d" % (coef, icpt, ddev, info["passes"], binfo["passes"]))
    if mix < 1 or K % 2 == 1:
        assert coef <= SAME_OPTIMUM_REL and icpt <= SAME_OPTIMUM_REL, (shape, mix, coef, icpt)
    assert ddev <= SAME_DEV_RATIO, (shape, mix, ddev)
    assert excess <= EXCESS_PASSES, (shape, mix, excess)


def test_restatement_on_the_other_gpu_inputs():
    """the user's lambdas, maxit = 1, a constant column and a class with a single member"""
    x, y = wr.problem(200, 6, 5, seed=2)
    check_restatement(x, y, 5, tm.NONMONOTONE, 0.5, True, True, "user lambdas")
    x, y = wr.problem(200, 6, 5, seed=3)
    lam = wr.automatic_lambdas(x, y, 5, 0.5, True, 5, 1e-2)
    _, _, _, short = wr.numpy_wide_mnewton_path(x, y, 5, lam, 0.5, thresh=1e-14, maxit=1)
    assert short["codes"][1:] == [1] * 4
    x, y = wr.problem(160, 5, 4, seed=5)
    x[:, 2] = 3.0
    for mix in wr.MIXES:
        for standardize in (True, False):
            lam = wr.automatic_lambdas(x, y, 4, mix, standardize, 5, 1e-2)
            _, beta, _, _ = check_restatement(x, y, 4, lam, mix, standardize, True, ("constant column", mix, standardize))
            assert (beta[:, 2] == 0.0).all()
    x, y = wr.problem(120, 4, 3, seed=6)
    y[y == 2] = 1.0
    y[7] = 2.0
    lam = wr.automatic_lambdas(x, y, 3, 0.5, True, 5, 1e-2)
    check_restatement(x, y, 3, lam, 0.5, True, True, "single member")


def test_lambda_max_first_is_exactly_zero():
    x, y = tm.iris()
    for intercept, standardize in wr.ALL_SETTINGS:
        for mix in (1.0, 0.5):
            lam = wr.automatic_lambdas(x, y, 3, mix, standardize, 4, 1e-4)
            a0, beta, dev, info = wr.numpy_wide_mnewton_path(x, y, 3, lam, mix, standardize, intercept)
            assert (beta[:, :, 0] == 0.0).all() and info["codes"][0] == 0, (intercept, standardize, mix)
