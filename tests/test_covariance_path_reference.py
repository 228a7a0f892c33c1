"""The reference of the covariance path kernels (tests/covariance_path_reference.py) on the CPU: nothing here needs a GPU.

  * the float64 restatement passes checks A to E on every committed case in three summation orders of the rebuild
    (sequential, pairwise, and the kernel's: ascending, a fused multiply-add per term), so the bounds hold for an honest
    implementation whatever its order;
  * the preconditions of D and E hold on every committed case (the reference asserts them itself: a case that is too close to
    a decision fails here, with the reference's own message, before it can fail on a device);
  * the re-screen inputs do re-screen: a second screen adds to a converged list;
  * every wrong version of the restatement (MUTANTS, CV_MUTANTS) fails at least one of A to E on at least one committed case:
    the table of which check caught which is printed (run with -s; profiles/covariance_path_mutants.txt keeps it)."""
import re
from types import SimpleNamespace

import numpy as np
import pytest

import covariance_path_reference as P

ORDERS = ["sequential", "pairwise", "kernel"]
LIMITS = P.limit_cases()
_built = {}


def built(spec):
    """(case, models, the cache of the reference's own runs), once per case"""
    key = P.case_id(spec)
    if key not in _built:
        case = P.build_case(spec)
        _built[key] = (case, P.host_models(case), {})
    return _built[key]


@pytest.mark.parametrize("spec", P.all_cases(), ids=P.case_id)
def test_the_restatement_passes_every_check_in_three_orders(spec):
    case, models, cache = built(spec)
    for order in ORDERS:
        P.check_case(case, P.restated(case, models[0], order=order), models, cache=cache)
    if "rescreen" in spec[5]:
        screens = cache[(1e-7, 1000)][1].screens_ld
        assert screens.max() >= 3, f"{case.name}: no second screen adds to a converged list: screens {screens.tolist()}"


@pytest.mark.parametrize("spec", LIMITS, ids=P.case_id)
def test_the_limit_cases_pass_checks_a_b_and_d(spec):
    case = P.build_case(spec)
    models = P.host_models(case)
    P.check_case(case, P.restated(case, models[0]), models, limit=True)


def test_the_group_limits_are_the_library_s():
    import wmcovariance_reference as wm
    assert P.mcov_max_features(2) == 195 and P.mcov_max_features(10) == 174 and wm.max_features(2) == wm.LIMITS[2]


# ---- the mutants ----
# where each is looked for, in this order, until a check catches it (small cases first)
SMALL = [("cov", 60, 9, 1, 0.5, {}), ("cov", 60, 9, 1, 0.0, {}), ("cov", 60, 2, 1, 0.5, {}), ("mcov", 60, 9, 3, 1.0, {}), ("mcov", 60, 9, 3, 0.0, {}),
         ("wcov", 65, 31, 1, 0.5, {}), ("wcov", 65, 33, 1, 0.0, {}), ("wcov", 65, 65, 1, 0.5, {}), ("wmcov", 63, 15, 4, 0.0, {}), ("wmcov", 63, 17, 4, 0.5, {}),
         ("wcov", 50, 300, 1, P.RESCREEN_MIX["wcov"], dict(rescreen=True)), ("wmcov", 50, 80, 2, P.RESCREEN_MIX["wmcov"], dict(rescreen=True))]
assert all(P.case_id(s) in {P.case_id(c) for c in P.all_cases()} for s in SMALL), "the mutants are looked for on committed cases only"
WHERE = {"no_second_screen": [s for s in SMALL if "rescreen" in s[5]], "tail_not_moved": [s for s in SMALL if s[2] % 2 == 1],
         "row_j_not_moved": [s for s in SMALL if s[0] in ("mcov", "wmcov")], "group_shrink_from_w": [s for s in SMALL if s[0] in ("mcov", "wmcov")],
         "group_norm_skips_response_0": [s for s in SMALL if s[0] in ("mcov", "wmcov")],
         "sweeps_count_screens": [s for s in SMALL if s[0] in ("wcov", "wmcov")], "max_iter_per_screen": [s for s in SMALL if s[0] in ("wcov", "wmcov")],
         "list_descending": [s for s in SMALL if s[0] in ("wcov", "wmcov")]}
_table = []


def caught_by(message):
    m = re.search(r": ([A-E]): ", message)
    return m.group(1) if m else "?"


def hunt(mutant, specs, forced_ridge=False):
    """the first case on which checks reject the mutant, with all the checks that do; a precondition is not a catch"""
    for spec in specs:
        case, models, cache = built(spec)
        if forced_ridge:
            if case.ridge or case.blocks:
                continue
            case, cache = SimpleNamespace(**{**vars(case), "ridge": True, "name": case.name + " ridge functor with an l1 term"}), {}
        failures = []
        try:
            with np.errstate(all="ignore"):          # (a mutant may diverge: its NaN is a catch of check A)
                P.check_case(case, P.restated(case, models[0], wrong=mutant), models, cache=cache, failures=failures)
        except P.Precondition:
            continue
        if failures:
            return " ".join(sorted({caught_by(m) for m in failures})), case.name, failures[0]
    return None


@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_every_mutant_is_caught(mutant):
    # the ridge functor never sees an l1 term from a fit (mix = 0 makes it 0), so "the ridge functor thresholds" shows only
    # where the restatement is handed one: the one-response committed cases with the functor forced
    got = hunt(mutant, WHERE.get(mutant, SMALL), forced_ridge=mutant == "ridge_thresholded")
    assert got is not None, f"no check catches the mutant {mutant}: a gap in the checks"
    _table.append((mutant, got[0], got[1]))
    print(f"mutant {mutant}: caught by check {got[0]} on {got[1]}: {got[2][:160]}")


def test_the_forced_ridge_functor_passes_when_right():
    """the case the ridge_thresholded mutant is caught on is one the right restatement passes"""
    case, models, _ = built(SMALL[0])
    forced = SimpleNamespace(**{**vars(case), "ridge": True, "name": case.name + " ridge functor with an l1 term"})
    P.check_case(forced, P.restated(forced, models[0]), models, cache={})


CV_FORMS = P.CV_FORMS


def cv_run(case, fields, wrong=None):
    models, pen_a, pen_b, ridge = fields

    def run(tol, max_iter):
        return P.run_cv([m[0] for m in models], pen_a, pen_b, ridge, tol, max_iter, blocks=case.blocks, listed=case.listed, wrong=wrong,
                        order="kernel" if case.listed else "sequential")
    return run


@pytest.mark.parametrize("form,n,p,K", CV_FORMS)
@pytest.mark.parametrize("train_on", ["fold", "rest"])
def test_the_cross_validation_restatement_passes_per_job(form, n, p, K, train_on):
    case = P.cv_case(form, n, p, K)
    fields = P.cv_host_fields(case, train_on)
    P.check_cv(case, cv_run(case, fields), lambda o: fields, what=f"cv {form} {train_on}")


@pytest.mark.parametrize("mutant", P.CV_MUTANTS)
def test_every_cross_validation_mutant_is_caught(mutant):
    got = None
    for form, n, p, K in CV_FORMS:
        case = P.cv_case(form, n, p, K)
        fields = P.cv_host_fields(case, "fold")
        try:
            P.check_cv(case, cv_run(case, fields, wrong=mutant), lambda o: fields, what=f"cv {form} fold")
        except P.Precondition:
            continue
        except AssertionError as e:
            got = (caught_by(str(e)), f"cv {form} fold", str(e))
            break
    assert got is not None, f"no check catches the mutant {mutant}: a gap in the checks"
    _table.append((mutant, got[0], got[1]))
    print(f"mutant {mutant}: caught by check {got[0]} on {got[1]}: {got[2][:160]}")


def test_print_the_table_of_mutants():
    """(after the two tests above in file order) the table profiles/covariance_path_mutants.txt keeps"""
    print("\nmutant                          checks    case")
    for mutant, check, case in _table:
        print(f"{mutant:<32}{check:<10}{case}")
    assert {m for m, _, _ in _table} >= set(P.MUTANTS) | set(P.CV_MUTANTS) or len(_table) == 0      # (a partial run prints what it has)
