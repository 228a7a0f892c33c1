"""The direct modes' rule (csrc/fit_plan.hpp: plan_fit) and their LDS budgets (csrc/covariance.hpp, newton.hpp, mnewton.hpp,
wide_layout.hpp), checked by what the compiled headers do: a stand-alone host program built with g++, no GPU.

Refusals: every rung of every mode's ladder, the return code and the whole message compared with
tests/golden/direct_plan_refusals.tsv, which the same program recorded from the commit before the six blocks of plan_fit
became one (python tests/test_direct_plan_host.py RECORD <csrc of that commit> rewrites it).  Budgets: the values of the
constexpr functions, against the numpy restatements."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sgdnet_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "direct_plan_refusals.tsv")

# include/sgdnet_hip.h
GAUSSIAN, BINOMIAL, MULTINOMIAL, MGAUSSIAN = 0, 1, 2, 3
MODES = {"covariance": 3, "newton": 4, "mcovariance": 5, "mnewton": 6, "wcovariance": 7, "wnewton": 8}
EUNSUPPORTED = -5
DEVICE = 3                                                      # (an accepted plan runs on control.device)


def case(mode, family, K, n, p, sparse=False, n_gpus=1, debug=0, type_multinomial=0):
    return dict(mode=mode, family=family, K=K, n=n, p=p, sparse=sparse, n_gpus=n_gpus, debug=debug, type_multinomial=type_multinomial)


def ladder(mode, family, other_family, K, limit, dense_copy=None, responses=(), tag=""):
    """One mode's rungs in the order plan_fit asks them, each broken alone, dense and sparse; then several broken at once
    (the first rung speaks); then the accepted plans at the limit and at one feature.  responses: (name, fields) of the
    rungs between the family's and the limit's."""
    n, few = 100, min(5, limit)     # (few: a feature count within every limit, so that the rung asked about is the one that speaks)
    out = []
    for sparse in (False, True):
        out.append(("family", case(mode, other_family, K, n, few, sparse)))
        for name, kw in responses:
            out.append((name, case(mode, family, kw.get("K", K), n, few, sparse, type_multinomial=kw.get("type_multinomial", 0))))
        out.append(("limit", case(mode, family, K, n, limit + 1, sparse)))
        out.append(("n_gpus", case(mode, family, K, n, few, sparse, n_gpus=2)))
        out.append(("debug", case(mode, family, K, n, few, sparse, debug=1)))
        out.append(("limit+n_gpus+debug", case(mode, family, K, n, limit + 1, sparse, n_gpus=2, debug=1)))
        out.append(("all", case(mode, other_family, responses[0][1].get("K", K) if responses else K, n, limit + 1, sparse, n_gpus=2, debug=1)))
        out.append(("accepted", case(mode, family, K, n, limit, sparse)))
        out.append(("accepted-1", case(mode, family, K, n, 1, sparse)))
    if dense_copy:
        rows, cols = dense_copy
        out.append(("dense copy", case(mode, family, K, rows, cols, True)))
        out.append(("dense copy+debug", case(mode, family, K, rows, cols, True, debug=1)))
        out.append(("dense copy: dense x", case(mode, family, K, rows, cols, False)))
        out.append(("dense copy: at the bound", case(mode, family, K, (1 << 30) // 8 // cols, cols, True)))
    return [("%s/%s/%s%s" % (mode, name, "sparse" if c["sparse"] else "dense", tag), c) for name, c in out]


def cases():
    out = []
    out += ladder("covariance", GAUSSIAN, BINOMIAL, 1, 198, responses=[("n_classes", {"K": 2})])
    out += ladder("wcovariance", GAUSSIAN, MGAUSSIAN, 1, 4531, responses=[("n_classes", {"K": 2})])
    out += ladder("newton", BINOMIAL, GAUSSIAN, 1, 198, responses=[("n_classes", {"K": 3})])
    # the dense copy of test_gpu_wnewton.py: 70 000 x 2000 x 8 bytes is more than 1 GiB
    out += ladder("wnewton", BINOMIAL, MULTINOMIAL, 1, 5819, dense_copy=(70000, 2000), responses=[("n_classes", {"K": 2})])
    for K, limit, tag in ((2, 195, ""), (10, 174, "/K10"), (96, 63, "/K96")):
        out += ladder("mcovariance", MGAUSSIAN, GAUSSIAN, K, limit, tag=tag)
    for K, limit, tag in ((2, 98, ""), (3, 65, "/K3"), (99, 1, "/K99")):
        out += ladder("mnewton", MULTINOMIAL, BINOMIAL, K, limit, dense_copy=(2_000_000, limit) if K == 2 else None, tag=tag,
                      responses=[("K = 1", {"K": 1}), ("K = 100", {"K": 100}), ("K = 0", {"K": 0}), ("type_multinomial", {"type_multinomial": 1})])
    assert len({name for name, _ in out}) == len(out)
    return out


PROGRAM = '''#include "fit_plan.hpp"
#include <cstdio>
using namespace sgdnet;
static void run(const char* name, int mode, int family, int K, long long n, long long p, int sparse, int n_gpus, int debug, int tm) {
  sgdnet_control c{};
  c.mode = mode; c.family = family; c.n_classes = K; c.n_gpus = n_gpus; c.debug = debug; c.type_multinomial = tm;
  c.device = %d; c.elasticnet_mix = 0.5;
  FitFacts f;
  f.ctl = &c; f.sparse = sparse != 0; f.n = n; f.p = p; f.n_devices = 8;
  const FitPlan P = plan_fit(f);
  printf("%%s\\t%%d\\t%%s\\n", name, P.rc, P.error.c_str());
  // what the driver reads of an accepted plan
  if (!P.rc)
    printf("+\\t%%d\\t%%zu %%d\\t%%zu %%lld %%lld\\n", P.mode, P.rank_dev.size(), P.rank_dev.empty() ? -1 : P.rank_dev[0], P.rank_lo.size(),
           P.rank_lo.empty() ? -1ll : (long long)P.rank_lo.front(), P.rank_lo.empty() ? -1ll : (long long)P.rank_lo.back());
}
int main() {
%s  return 0;
}
'''


def compile_and_run(tmp, name, text, csrc=CSRC):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler builds the rest of the tests' helpers too"
    src, exe = os.path.join(tmp, name + ".cpp"), os.path.join(tmp, name)
    with open(src, "w") as f:
        f.write(text)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", csrc, src, "-o", exe])
    return subprocess.check_output([exe], text=True)


def run_plans(tmp, csrc=CSRC):
    calls = "".join('  run("%s", %d, %d, %d, %dll, %dll, %d, %d, %d, %d);\n'
                    % (name, MODES[c["mode"]], c["family"], c["K"], c["n"], c["p"], c["sparse"], c["n_gpus"], c["debug"], c["type_multinomial"])
                    for name, c in cases())
    return compile_and_run(str(tmp), "direct_plans", PROGRAM % (DEVICE, calls), csrc)


def test_every_refusal_of_every_direct_mode_is_the_recorded_one(tmp_path):
    got = run_plans(tmp_path).split("\n")
    # rc and message, byte for byte
    assert [l for l in got if l and not l.startswith("+")] == open(GOLDEN).read().split("\n")[:-1]
    by_name, accepted = {}, {}
    for i, line in enumerate(got):
        if line and not line.startswith("+"):
            name, rc, msg = line.split("\t")
            by_name[name] = (int(rc), msg)
            if int(rc) == 0:
                accepted[name] = got[i + 1]
    assert len(by_name) == len(cases())
    for name, c in cases():
        rc, msg = by_name[name]
        rung = name.split("/")[1]
        if rung.startswith("accepted") or rung in ("dense copy: dense x", "dense copy: at the bound"):
            assert rc == 0 and msg == "", name
            # the mode asked for, on control.device, all the samples in one rank
            assert accepted[name] == "+\t%d\t1 %d\t2 0 %d" % (MODES[c["mode"]], DEVICE, c["n"]), name
        else:
            assert rc == EUNSUPPORTED and msg.startswith("mode = %s needs " % c["mode"]), name
            assert "%d features (limit " % c["p"] in msg and ("%d samples" % c["n"] in msg) == (c["mode"] in ("wnewton", "mnewton")), name
            assert ("n_classes %d" % c["K"] in msg) == (c["mode"] != "newton"), name
    # the rungs in their order: what is broken first speaks
    needs = lambda name: by_name[name][1].split(" needs ")[1].split(":")[0]
    starts = {"family": "family = ", "limit": "no more features than ", "n_gpus": "one GPU", "debug": "debug = 0", "dense copy": "the dense copy"}
    for name, _ in cases():                                     # every case named after a rung records that rung
        rung = name.split("/")[1]
        assert rung not in starts or needs(name).startswith(starts[rung]), name
    for mode in ("covariance", "wcovariance", "newton", "wnewton"):
        assert needs(mode + "/all/dense") == needs(mode + "/family/dense") == "family = " + ("gaussian" if "cov" in mode else "binomial")
        assert needs(mode + "/n_classes/sparse") == "one response (n_classes = 1)"
        assert needs(mode + "/limit+n_gpus+debug/dense") == needs(mode + "/limit/dense") == "no more features than sgdnet_%s_max_features()" % mode
        assert needs(mode + "/n_gpus/sparse") == "one GPU (n_gpus <= 1)" and needs(mode + "/debug/dense").startswith("debug = 0 (")
    assert needs("mnewton/K = 1/dense") == needs("mnewton/K = 100/sparse") == needs("mnewton/K = 0/dense") == "2 to 99 classes"
    assert needs("mnewton/type_multinomial/dense") == "the ungrouped penalty (type_multinomial = 0)"
    assert needs("mnewton/all/dense") == "family = multinomial" and needs("mcovariance/all/sparse") == "family = mgaussian"
    for mode in ("wnewton", "mnewton"):
        assert needs(mode + "/dense copy/sparse") == "the dense copy of a sparse x (n_samples x n_features x 8 bytes) within 1 GiB"
        assert needs(mode + "/dense copy+debug/sparse").startswith("debug = 0 (")
    assert "70000 samples, 2000 features" in by_name["wnewton/dense copy/sparse"][1]


BUDGETS = '''#include "fit_plan.hpp"
#include <cstdio>
using namespace sgdnet;
int main() {
  printf("%d %d %d %d\\n", kCovMaxFeatures, kNewtonMaxFeatures, kWcovMaxFeatures, kWnewtonMaxFeatures);
  printf("%d %d\\n", kCovLdsBytes, kWnewtonLdsBytes);
  for (int P = 1; P <= 5822; ++P) printf("%d %d\\n", wcov_state_bytes(P), wnewton_state_bytes(P));
  const int Kc[] = {-3, 0, 1, 2, 3, 5, 10, 16, 32, 64, 95, 96, 6826, 6827, 2147483647};
  for (int K : Kc) printf("%d ", mcov_max_features(K));
  printf("\\n");
  const int Kn[] = {-3, 0, 1, 2, 3, 4, 5, 10, 99, 100, 101, 199, 200, 2147483647};
  for (int K : Kn) printf("%d ", mnewton_max_features(K));
  printf("\\n");
  for (int m = 0; m <= 9; ++m) printf("%d", is_direct_mode(m) ? 1 : 0);
  printf("\\n");
  return 0;
}
'''


def test_lds_budgets_are_the_restated_ones(tmp_path):
    import wcovariance_reference as wc
    import wnewton_reference as wn
    import test_wcovariance_host as wch
    out = compile_and_run(str(tmp_path), "budgets", BUDGETS).split("\n")
    assert [int(v) for v in out[0].split()] == [198, 198, 4531, 5819]
    assert wc.LIMIT == 4531 and wn.LIMIT == 5819
    assert [int(v) for v in out[1].split()] == [160 * 1024, wn.LDS_BYTES]
    for P in range(1, 5823):
        cov, newton = (int(v) for v in out[1 + P].split())
        assert cov == wch.state_bytes(P) and newton == wn.state_bytes(P), P
    # the limits are where the budgets end
    assert wch.state_bytes(4531) <= 160 * 1024 < wch.state_bytes(4532)
    assert wn.state_bytes(5819 + 1) <= wn.LDS_BYTES < wn.state_bytes(5819 + 2)
    # the K that test_mcovariance_host.py and test_mnewton_host.py name
    assert [int(v) for v in out[5824].split()] == [0, 0, 198, 195, 193, 187, 174, 159, 127, 86, 64, 63, 1, 0, 0]
    assert [int(v) for v in out[5825].split()] == [0, 0, 0, 98, 65, 48, 38, 18, 1, 0, 0, 0, 0, 0]
    assert out[5826] == "0001111110"                          # modes 3 .. 8 and no other


if __name__ == "__main__" and sys.argv[1:2] == ["RECORD"]:
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        lines = [l for l in run_plans(tmp, sys.argv[2]).split("\n") if l and not l.startswith("+")]
    with open(GOLDEN, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("recorded %d plans from %s" % (len(lines), sys.argv[2]))
