"""SGDNET_MODE_WMCOVARIANCE on the CPU: the header, the binding, the package and the shim agree; the feature limit is the
LDS budget and the column cap written in csrc/covariance.hpp; the plan accepts and refuses the mode rung by rung; and the
algorithm restated in numpy (tests/wmcovariance_reference.py) reaches the project's optimality bound on every input
tests/test_gpu_wmcovariance.py gives the device outside the limit shapes, agrees with the full block sweeps of
tests/test_gpu_mcovariance.py::numpy_block_cd_path within the pinned distance, and goes back to the screen on the
re-screen input -- so the bounds ask nothing of the device that the method and f64 do not give."""
import os
import re

import numpy as np
import pytest

import test_direct_plan_host as dp
import wmcovariance_reference as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE = 9
K_PINNED = [1, 2, 3, 10, 96]
K_NOTHING = [-3, 0, 4093, 4531, 4532, 2147483647]     # no response; one feature's state beyond the LDS (from 4093 on); no overflow


# ---- the header, the binding, the package, the shim ----

def test_header_binding_package_and_shim_agree():
    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sgdnet_hip.h")).read()
    assert int(re.search(r"#define SGDNET_MODE_WMCOVARIANCE\s+(\d+)", hdr).group(1)) == _lib.MODE_WMCOVARIANCE == MODE
    assert int(re.search(r"#define SGDNET_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 6
    assert re.search(r"int sgdnet_wmcovariance_max_features\(int n_responses\);", hdr) and '"wmcovariance_width"' in hdr
    assert "sgdnet_wmcovariance_max_features" in _lib.EXPORTS
    assert "sgdnet_wmcovariance" in sa.__all__ and "wmcovariance_max_features" in sa.__all__
    assert _lib.MODES == {"exact": 0, "batched": 1, "auto": 2, "covariance": 3}      # sgdnet(mode=...) does not reach mode 9
    shim = open(os.path.join(ROOT, "shim", "sgdnet_shim.c")).read()
    assert '"wmcovariance") == 0) c->mode = SGDNET_MODE_WMCOVARIANCE' in shim


def test_mode_string_is_not_one_of_sgdnet():
    import sgdnet_amd as sa
    x = np.random.default_rng(0).standard_normal((20, 3))
    y = np.column_stack([x[:, 0] + 1.0, x[:, 1] - 1.0])
    with pytest.raises(ValueError, match="mode must be one of"):
        sa.sgdnet(x, y, family="mgaussian", nlambda=3, mode="wmcovariance")
    if sa.load().sgdnet_device_count() == 0:
        # sgdnet_wmcovariance passes the argument mapping and reaches the backend, which has no device to run on
        with pytest.raises(sa.SgdnetError) as e:
            sa.sgdnet_wmcovariance(x, y, nlambda=3)
        assert e.value.code == -2


def test_width_option_is_one_of_the_library():
    import sgdnet_amd as sa
    assert sa.get_option("wmcovariance_width") == 0
    with sa.option("wmcovariance_width", 1024):
        assert sa.get_option("wmcovariance_width") == 1024
    with pytest.raises(sa.SgdnetError):
        sa.set_option("wmcovariance_width", 2048)
    assert sa.get_option("wmcovariance_width") == 0


# ---- the limit ----

LIMITS = '''#include "fit_plan.hpp"
#include <cstdio>
using namespace sgdnet;
int main() {
  const int Ks[] = {%s};
  for (int K : Ks) printf("%%d %%d\\n", K, wmcov_max_features(K));
  for (int K : {1, 2, 3, 10, 96})
    for (int p : {1, 2, 3, 104, 105, 950, 951, 2722, 2723, 3709, 3710, 4531}) printf("%%lld\\n", (long long)wmcov_state_bytes(p, K));
  printf("%%d %%d %%d\\n", kWideLdsBytes, kWcovMaxFeatures, plans_direct(%d) ? 1 : 0);
  return 0;
}
'''


def test_feature_limit_is_the_lds_budget_and_the_column_cap(tmp_path):
    ks = K_PINNED + K_NOTHING + [4092]
    out = dp.compile_and_run(str(tmp_path), "wmcov_limits", LIMITS % (", ".join(str(k) for k in ks), MODE)).split("\n")
    got = dict(tuple(int(v) for v in line.split()) for line in out[:len(ks)])
    for K in ks:
        assert got[K] == wm.max_features(K), K                                      # the header's constexpr against the restated formula
    assert {K: got[K] for K in K_PINNED} == wm.LIMITS == {1: 4531, 2: 3709, 3: 2722, 10: 950, 96: 104}
    assert all(got[K] == 0 for K in K_NOTHING) and got[4092] == 2
    states = [int(v) for v in out[len(ks):len(ks) + 60]]
    assert states == [wm.state_bytes(p, K) for K in (1, 2, 3, 10, 96) for p in (1, 2, 3, 104, 105, 950, 951, 2722, 2723, 3709, 3710, 4531)]
    assert [int(v) for v in out[len(ks) + 60].split()] == [wm.LDS_BYTES, wm.MAX_COLUMNS - 1, 1]
    for K, p in wm.LIMITS.items():
        # the limit is where the LDS ends -- or, for one response, where the moments pass's columns end
        assert wm.fits(p, K) and not wm.fits(p + 1, K)
        assert (wm.state_bytes(p + 1, K) > wm.LDS_BYTES) == (K > 1) and (p + 1 + K > wm.MAX_COLUMNS) == (K == 1)
    assert wm.LIMITS[2] >= 2048 and wm.LIMITS[10] >= 512                              # what include/sgdnet_hip.h promises
    hdr = re.sub(r"[\s*]+", " ", open(os.path.join(ROOT, "include", "sgdnet_hip.h")).read())
    assert "4531 at K = 1, 3709 at K = 2, 2722 at K = 3, 950 at K = 10, 104 at K = 96" in hdr
    cov = open(os.path.join(ROOT, "sgdnet_amd", "csrc", "covariance.hpp")).read()
    assert "wmcov_max_features(2) == 3709 && wmcov_max_features(3) == 2722" in cov
    assert "wmcov_max_features(10) == 950 && wmcov_max_features(96) == 104" in cov


def test_library_reports_the_same_limits():
    import sgdnet_amd as sa
    for K in K_PINNED + K_NOTHING + [4092]:
        assert sa.wmcovariance_max_features(K) == wm.max_features(K), K


# ---- the plan ----

def test_plan_accepts_and_refuses_rung_by_rung(tmp_path):
    modes = dict(dp.MODES, wmcovariance=MODE)
    cases = []
    for K, tag in ((2, ""), (10, "/K10")):
        cases += dp.ladder("wmcovariance", dp.MGAUSSIAN, dp.GAUSSIAN, K, wm.LIMITS[K], tag=tag)
    cases.append(("mcovariance/limit/dense", dp.case("mcovariance", dp.MGAUSSIAN, 2, 100, 196)))
    calls = "".join('  run("%s", %d, %d, %d, %dll, %dll, %d, %d, %d, %d);\n'
                    % (name, modes[c["mode"]], c["family"], c["K"], c["n"], c["p"], c["sparse"], c["n_gpus"], c["debug"], c["type_multinomial"])
                    for name, c in cases)
    got = dp.compile_and_run(str(tmp_path), "wmcov_plans", dp.PROGRAM % (dp.DEVICE, calls)).split("\n")
    by_name, accepted = {}, {}
    for i, line in enumerate(got):
        if line and not line.startswith("+"):
            name, rc, msg = line.split("\t")
            by_name[name] = (int(rc), msg)
            if int(rc) == 0:
                accepted[name] = got[i + 1]
    assert len(by_name) == len(cases)
    needs = lambda name: by_name[name][1].split(" needs ")[1].split(":")[0]
    starts = {"family": "family = mgaussian", "limit": "no more features than sgdnet_wmcovariance_max_features(n_classes)",
              "n_gpus": "one GPU (n_gpus <= 1)", "debug": "debug = 0 (", "limit+n_gpus+debug": "no more features than ", "all": "family = mgaussian"}
    for name, c in cases[:-1]:
        rc, msg = by_name[name]
        rung = name.split("/")[1]
        if rung.startswith("accepted"):
            # mode 9 on control.device, all the samples in one rank
            assert rc == 0 and msg == "" and accepted[name] == "+\t%d\t1 %d\t2 0 %d" % (MODE, dp.DEVICE, c["n"]), name
        else:
            assert rc == dp.EUNSUPPORTED and msg.startswith("mode = wmcovariance needs "), name
            assert needs(name).startswith(starts[rung]), (name, msg)                # the rungs speak in order: what is broken first
            assert "n_classes %d, %d features (limit %d)" % (c["K"], c["p"], wm.LIMITS[c["K"]]) in msg and "samples" not in msg, name
    assert "3710 features (limit 3709)" in by_name["wmcovariance/limit/sparse"][1]
    assert "951 features (limit 950)" in by_name["wmcovariance/limit/dense/K10"][1]
    # the narrow mode is not handed on to the wide one: 196 features at K = 2 are refused with its own text
    assert by_name["mcovariance/limit/dense"] == (dp.EUNSUPPORTED, "mode = mcovariance needs no more features than "
                                                  "sgdnet_mcovariance_max_features(n_classes): family 3, n_classes 2, 196 features (limit 195), n_gpus 1, debug 0")


# ---- the restatement ----

@pytest.fixture(scope="module")
def paths():
    """the restatement and the full block sweeps on every input, once: (what, x, y, lambdas, mix, settings, wide, full)"""
    out = []
    for what, x, y, lam, mix, standardize, intercept, standardize_response in wm.inputs():
        wide = wm.numpy_wide_group_path(x, y, lam, mix, standardize, intercept, standardize_response)
        full = wm.numpy_block_cd_path(x, y, lam, mix, standardize, intercept, standardize_response)
        out.append((what, x, y, np.asarray(lam, dtype=float), mix, (standardize, intercept, standardize_response), wide, full))
    return out


def test_restatement_is_optimal_on_the_gpu_inputs(paths):
    worst = 0.0
    for what, x, y, lam, mix, (standardize, intercept, standardize_response), wide, _ in paths:
        a0, beta, dev_ratio, sweeps, screens, _, unconverged = wide
        assert not unconverged.any() and sweeps.max() < wm.MAXIT and screens.min() >= 2, (what, sweeps, screens)
        k = wm.numpy_kkt(a0, beta, x, y, lam, mix, standardize, intercept, standardize_response)
        worst = max(worst, np.max(k["ratio"]), np.max(k["intercept"] / lam))
        assert (k["ratio"] <= wm.KKT_BOUND).all() and (k["intercept"] <= wm.KKT_BOUND * lam).all(), (what, k["ratio"], k["intercept"])
        ref = wm.tm.numpy_dev_ratio(a0, beta, x, y, standardize, intercept, standardize_response)
        assert np.abs(dev_ratio - ref).max() <= wm.DEV_TOL, what
    print("worst KKT ratio of the restatement %.3g over %d inputs" % (worst, len(paths)))


def test_restatement_agrees_with_the_full_sweeps(paths):
    """The pins of wmcovariance_reference.py, measured here: they are what was seen, rounded up"""
    rel = dev = 0.0
    for what, _, _, _, _, _, wide, full in paths:
        scale = np.abs(full[1]).max()
        if scale > 0.0:
            rel = max(rel, np.abs(wide[1] - full[1]).max() / scale, np.abs(wide[0] - full[0]).max() / max(scale, np.abs(full[0]).max()))
        dev = max(dev, np.abs(wide[2] - full[2]).max())
    print("restatement vs full block sweeps: coefficients / max|beta| = %.3g, dev_ratio %.3g" % (rel, dev))
    assert rel <= wm.BLOCK_CD_REL and dev <= wm.BLOCK_CD_DEV


def test_rescreen_input_sends_the_algorithm_back_to_the_screen(paths):
    """At some lambda the list converges, the second screen adds a block, and only a later one adds nothing: three screens
    at least (two is the minimum of every lambda)."""
    what, _, _, _, _, _, wide, _ = paths[-1]
    assert what == ("re-screen",)
    screens, added = wide[4], wide[5]
    assert screens.min() >= 2 and screens.max() >= 3, screens
    assert any(len(a) >= 3 and a[1] >= 1 for a in added), added
