"""The path kernels of one fit of the covariance family (sgdnet_amd/csrc/covariance.hip: cov_path_kernel,
cov_group_path_kernel<64|256>, cov_wide_path_kernel<256|1024, ahead 0|1>, cov_wide_group_path_kernel<256|1024>) sweep by sweep,
through sgdnet_covariance_path_probe, against tests/covariance_path_reference.py (which says what checks A to E are and where
their bounds come from; tests/test_covariance_path_reference.py shows on the CPU that they hold for a right implementation and
reject seventeen wrong ones).  tests/test_gpu_covariance_passes.py checks the stages BEFORE the path kernel.

Every reference starts from what the kernel itself was handed (the tapped M, or S, diag S and c~, and the tapped tol and
max_iter), so a failure names the path kernel.  The shapes:
  cov_path_kernel            p = 1, 2; 63, 64, 65 around the wavefront; 198 = sgdnet_covariance_max_features(); a sparse x; a
                             constant column with and without an l2 term
  cov_group_path_kernel      (p, K) = (1, 2), (9, 3), (16, 4): 64 entries, the last shape of the 64-lane rule; (13, 5): 65;
                             (86, 3): 258, one past a stride of 256; (5, 70): K above a wavefront; the limits of K = 2 and 10.
                             Both widths forced on every shape: equal bytes
  cov_wide_path_kernel       wcovariance_reference.WIDTH_SHAPES' p and 1025; 1537, 1538: the look-ahead instance, odd and
                             even (chosen by wcov_path_ahead(p): reached by shape); the re-screen input; 4531, the limit, with
                             two lambdas and checks A, B, D.  Both widths: equal bytes
  cov_wide_group_path_kernel wmcovariance_reference.SHAPES, the re-screen input, the limit of K = 2 (A, B, D).  Both widths.
                             (1537, 2) is not here: the kernel has no look-ahead instance (its only template parameter is the
                             width), so that shape is no instance of its own.
Each check prints the value closest to its bound (run with -s); profiles/covariance_path_passes.txt keeps one run's."""
import numpy as np
import pytest

import covariance_path_reference as P

pytestmark = pytest.mark.gpu

EINVAL = -1
WIDTHS = {"cov": (0,), "mcov": (64, 256), "wcov": (256, 1024), "wmcov": (256, 1024)}


@pytest.fixture(scope="module")
def probe():
    import torch  # noqa: F401  -- before libsgdnet_hip.so (sgdnet_amd/_lib.py)
    import sgdnet_amd
    L = sgdnet_amd.load()
    if L.sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    assert L.sgdnet_covariance_max_features() == P.COV_MAX_FEATURES and L.sgdnet_wcovariance_max_features() == P.WCOV_MAX_FEATURES
    assert L.sgdnet_mcovariance_max_features(2) == P.mcov_max_features(2) and L.sgdnet_mcovariance_max_features(10) == P.mcov_max_features(10)
    assert L.sgdnet_wmcovariance_max_features(2) == P.wmcov_max_features(2)
    from sgdnet_amd import diagnostics
    return diagnostics


def device(probe, case, width):
    """run(tol, max_iter, lam) of check_case on the device; every answer is kept, so a setting runs once per width"""
    kept = {}

    def run(tol, max_iter, lam):
        key = (tol, max_iter, np.asarray(lam).tobytes())
        if key not in kept:
            o = probe.covariance_probe(case.x, case.y, case.scale, case.mix, lam, wide=case.wide, multi=case.multi, tol=tol, max_sweeps=max_iter,
                                       width=width)
            assert o.tol[0] == tol and o.max_iter[0] == max_iter, "the kernel was handed another stopping rule than the probe was"
            assert o.sweeps.dtype == np.int64 and o.unconverged.dtype == np.int64
            if case.wide:
                P.check_pad(o.S)
            kept[key] = o
        return kept[key]
    return run, kept


def check_on_device(probe, spec, limit=False):
    case = P.build_case(spec)
    widths = WIDTHS[case.form]
    run, kept = device(probe, case, widths[0])
    models = P.models_of(case, run(P.REPLAY_TOL, 1, case.lam))
    P.check_case(case, run, models, limit=limit)
    for other in widths[1:]:
        again, _ = device(probe, case, other)
        for (tol, max_iter, lam), o in kept.items():
            P.same_bytes(again(tol, max_iter, np.frombuffer(lam)), o, f"{case.name}: widths {widths[0]} and {other} (tol {tol}, max_iter {max_iter})")
    return case, run


@pytest.mark.parametrize("spec", P.narrow_cases(), ids=P.case_id)
def test_cov_path_kernel(probe, spec):
    check_on_device(probe, spec)


@pytest.mark.parametrize("spec", P.group_cases(), ids=P.case_id)
def test_cov_group_path_kernel(probe, spec):
    check_on_device(probe, spec)


@pytest.mark.parametrize("spec", P.wide_cases(), ids=P.case_id)
def test_cov_wide_path_kernel(probe, spec):
    check_on_device(probe, spec)


@pytest.mark.parametrize("spec", P.wide_group_cases(), ids=P.case_id)
def test_cov_wide_group_path_kernel(probe, spec):
    check_on_device(probe, spec)


@pytest.mark.parametrize("spec", P.limit_cases(), ids=P.case_id)
def test_the_wide_feature_limits(probe, spec):
    check_on_device(probe, spec, limit=True)


def test_the_width_of_a_fit_is_one_of_the_two(probe):
    """width = 0 follows the rule of a fit: its bytes are those of the width the rule names"""
    for spec, rule in ((("mcov", 80, 16, 4, 0.0, {}), 64), (("mcov", 80, 13, 5, 0.5, {}), 256), (("wcov", 65, 257, 1, 0.5, {}), 256),
                       (("wmcov", 90, 1025, 3, 1.0, {}), 1024)):
        case = P.build_case(spec)
        by_rule, forced = device(probe, case, 0)[0](1e-7, 5, case.lam), device(probe, case, rule)[0](1e-7, 5, case.lam)
        P.same_bytes(by_rule, forced, f"{case.name}: width 0 and {rule}")


def test_the_probe_refuses_other_widths_and_no_sweeps(probe):
    from sgdnet_amd import SgdnetError
    case = P.build_case(("cov", 60, 9, 1, 0.5, {}))
    group = P.build_case(("mcov", 60, 9, 3, 1.0, {}))
    for c, kw in ((case, dict(width=64)), (case, dict(width=256)), (case, dict(wide=True, width=64)), (case, dict(wide=True, width=512)),
                  (group, dict(width=1024)), (group, dict(width=128)), (group, dict(wide=True, width=64)), (case, dict(max_sweeps=0)),
                  (group, dict(wide=True, max_sweeps=0))):
        with pytest.raises(SgdnetError) as e:
            probe.covariance_probe(c.x, c.y, c.scale, c.mix, c.lam, **kw)
        assert e.value.code == EINVAL and "sgdnet_covariance_path_probe: invalid argument" in str(e.value), kw


def test_the_old_probe_is_the_new_one_with_the_defaults(probe):
    """sgdnet_covariance_probe = sgdnet_covariance_path_probe(1e-7, 1000, 0): the tapped rule says so"""
    import ctypes as C
    from sgdnet_amd import _lib
    from sgdnet_amd.diagnostics import _cov_fields, check, dptr
    case = P.build_case(("cov", 60, 9, 1, 0.5, {}))
    xd, y = np.asfortranarray(case.x), np.asfortranarray(case.y.reshape(-1, 1))
    handle = C.c_void_p()
    check(_lib.load().sgdnet_covariance_probe(dptr(xd), None, case.n, case.p, dptr(y), 1, dptr(case.scale), 1, 0, 0, case.mix, len(case.lam),
                                              dptr(np.ascontiguousarray(case.lam)), 0, C.byref(handle)))
    old = _cov_fields(handle, {"tol": (1,), "max_iter": (1,), "W": (4, 9, 1), "G": (4, 9, 1), "sweeps": (4,), "unconverged": (4,)})
    assert old.tol[0] == 1e-7 and old.max_iter[0] == 1000
    P.same_bytes(old, probe.covariance_probe(case.x, case.y, case.scale, case.mix, case.lam), "the old entry and the new one's defaults")
