"""The checks of tests/covariance_passes_reference.py, proved on the CPU on the very inputs the GPU tests use
(tests/test_gpu_covariance_passes.py, tests/test_gpu_cv_covariance_passes.py): float64 restatements of every stage of the
covariance family, in three summation orders, pass every check; every wrong version (`wrong=`) fails a NAMED check on at
least one input; the lists of shapes meet the conditions they were chosen for; the constant-on-a-training-set rule
 covers every exactly-constant column and stays MARGIN away from every other, on these inputs and on those of
the pooling restatements of tests/test_cv_*_host.py (all but their 4531-feature shape); and the largest bound / sum|terms| per stage is printed (run with -s; profiles/covariance_passes.txt
has a copy), so that a vacuous bound would be visible.  No library is loaded."""
import functools
import re

import numpy as np
import pytest

import covariance_passes_reference as R
from newton_reference import SUMS

BIG = ("w65x1025",)       # one order only: a restatement of 65 x 1027^2 terms takes 15 s


def cv_cases():
    """name -> builder of every cross-validation input of the GPU tests"""
    c = {f"dense/{k}": (lambda k=k: R.cv_dense_case(k)) for k in list(R.CV_DENSE) + list(R.CV_WIDE)}
    c.update({f"dense-as-wide/{k}": (lambda k=k: R.cv_dense_case(k, wide=True)) for k in ("n63_Pa15", "n256_Pa31", "n1025_Pa33")})
    c.update({f"sparse/{k}": (lambda k=k: R.cv_sparse_case(k)) for k in R.CV_SPARSE})
    c.update({f"sparse-wide/{k}": (lambda k=k: R.cv_sparse_case(k, wide=True)) for k in ("s600", "s257_K2")})
    c["sparse/s600_desc"] = lambda: R.cv_sparse_case("s600", descending=True)
    c["sparse/empty"] = R.empty_sparse_cv_case
    c["loo37"] = R.loo_case
    c["loo37_wide"] = lambda: R.loo_case(wide=True)
    c["constant_response"] = R.constant_response_case
    c["constant_response_wide"] = lambda: R.constant_response_case(wide=True)
    for rest in (False, True):
        for multi in (False, True):
            for wide in (False, True):
                c[f"degenerate/{int(rest)}{int(multi)}{int(wide)}"] = lambda r=rest, m=multi, w=wide: R.degenerate_case(r, m, w)
    c["degenerate/unscaled"] = lambda: R.degenerate_case(False, True, False, standardize=False, standardize_response=False)
    return c


def single_cases():
    c = {f"dense/{k}": (lambda k=k: R.single_dense_case(k)) for k in R.SINGLE_DENSE}
    c["dense/uncentred"] = lambda: R.single_dense_case("n65_P31", centre=False)
    c["sparse/600"] = lambda: R.single_sparse_case(600)
    c["sparse/600_K3_wide"] = lambda: R.single_sparse_case(600, K=3, wide=True)
    c["sparse/257_desc"] = lambda: R.single_sparse_case(257, descending=True)
    c["sparse/257_uncentred"] = lambda: R.single_sparse_case(257, centre=False)
    c["sparse/1"] = lambda: R.single_sparse_case(1)
    c["sparse/empty"] = R.empty_sparse_single_case
    return c


CV, SINGLE = cv_cases(), single_cases()


@functools.lru_cache(maxsize=None)
def checked(kind, name):
    """every check on the float64 restatements of one input, in the three summation orders (the BIG case in one); returns the
    input's largest bound / sum|terms| per stage.  Cached: the ratio test below reads what the restatement tests computed,
    or computes it itself when it runs without them."""
    case = (CV if kind == "cv" else SINGLE)[name]()
    ratios = {}
    for order, fsum in SUMS.items():
        if case.name in BIG and order != "strided256":
            continue
        if kind == "cv":
            R.check_cv(R.restate_cv(case, fsum), case, ratios)
        else:
            R.check_single(R.restate_single(case, fsum), case, ratios)
    return ratios


@pytest.mark.parametrize("name", sorted(CV))
def test_cv_restatements_pass_every_check(name):
    checked("cv", name)


@pytest.mark.parametrize("name", sorted(SINGLE))
def test_single_restatements_pass_every_check(name):
    checked("single", name)


def test_bound_ratios_are_not_vacuous():
    """the largest bound / sum|terms| of each stage over every input.  gamma_n at n = 1025 is 1.1e-13; a deviation's and a
    product's rounding add 3 u; the assembly's re-centring is a dozen roundings."""
    worst = {}
    for kind, names in (("cv", sorted(CV)), ("single", sorted(SINGLE))):
        for name in names:
            for k, v in checked(kind, name).items():
                worst[k] = max(worst.get(k, 0.0), v)
    for k, v in sorted(worst.items()):
        print(f"largest bound / sum|terms|: {k}: {v:.3e}")
    assert 0 < worst["dense moments"] < 2e-13 and 0 < worst["sparse moments"] < 2e-13 and 0 < worst["total"] < 1e-14 and 0 < worst["assembly"] < 1e-12


# which inputs can show each wrong version, and the check that must name it
NAMED = {
    "raw_moments": r": moments of row set",
    "no_in_neither": r": moments of row set",
    "union_miscounted": r": moments of row set",
    "other_groups_rows": r": moments of row set",
    "dropped_last_step": r": corner: ",
    "chunk_to_neighbour": r": corner: ",
    "reduce_off_by_one": r": corner: ",
    "total_missing_last": r": total: ",
    "d_not_zeroed": r": Mt of set|: s, d of set",
    "sign_nTdd": r": scale of set",
    "sdy_before_recentre": r": sd_y of set|: ysd of set|: yy of set",       # (narrow K responses: sd_y shows in y~'y~ only)
    "n_for_nT": r": scale of set",
    "c_not_div_sdy": r": Mt of set|: c~_T of set",
    "shift_neighbour": r": mean of set|: nulldev of set|: s, d of set",
    "constant_response_kept": r": constant response: |: sd_y of set|: ysd of set|: yy of set",
    "nulldev_scaled": r": nulldev of set",
    "nonzero_pad": r": pad: ",
    "lower_unmirrored": r": S_T symmetric: ",
}
CANDIDATES = {
    "raw_moments": ["dense/mean1e6"],
    "no_in_neither": ["sparse/s600"], "union_miscounted": ["sparse/s600"], "other_groups_rows": ["sparse/s600"],
    "dropped_last_step": ["dense/n65_Pa17", "dense/n1025_Pa33"], "chunk_to_neighbour": ["dense/n1025_Pa33"],
    "reduce_off_by_one": ["dense/n1025_Pa33"], "total_missing_last": ["dense/n63_Pa15"],
    "d_not_zeroed": ["dense/n65_Pa17", "dense/w257x209_K2"], "sign_nTdd": ["dense/n63_Pa15"],
    "sdy_before_recentre": ["dense/n63_Pa15", "dense/n256_Pa31"], "n_for_nT": ["dense/n63_Pa15"],
    "c_not_div_sdy": ["dense/n63_Pa15", "dense/w65x209_K2"], "shift_neighbour": ["dense/n256_Pa31", "dense/w65x209_K2"],
    "constant_response_kept": ["constant_response", "degenerate/011"], "nulldev_scaled": ["dense/n256_Pa31"],
    "nonzero_pad": ["dense/w65x199"], "lower_unmirrored": ["dense/w65x199"],
}


@pytest.mark.parametrize("wrong", R.WRONG)
def test_every_wrong_version_fails_a_named_check(wrong):
    assert wrong in NAMED and wrong in CANDIDATES
    failed = []
    for name in CANDIDATES[wrong]:
        case = CV[name]()
        try:
            R.check_cv(R.restate_cv(case, SUMS["strided256"], wrong=wrong), case)
        except AssertionError as e:
            msg = str(e).split("\n")[0]
            assert re.search(NAMED[wrong], msg), f"{wrong} on {name} failed an unexpected check: {msg}"
            failed.append((name, msg))
    assert failed, f"{wrong}: no check noticed it on {CANDIDATES[wrong]}"
    print(f"{wrong}: {failed[0][1][:150]}")


def test_the_lists_meet_their_conditions():
    dense = {k: v for k, v in R.CV_DENSE.items()}
    pa = sorted({p + max(K, 1) + 1 for (n, p, K, *_) in dense.values()})
    assert {15, 16, 17, 31, 32, 33} <= set(pa), pa
    assert {n for (n, *_) in dense.values()} >= {1, 63, 64, 65, 256, 257, 1025}
    single = {p + max(K, 1) for (n, p, K, w) in R.SINGLE_DENSE.values() if not w}
    assert {15, 16, 17, 31, 32, 33} <= single and {n for (n, *_) in R.SINGLE_DENSE.values()} >= {1, 63, 64, 65, 256, 257, 1025}
    assert {p for (n, p, K, w) in R.SINGLE_DENSE.values() if w} == {199, 208, 209, 1025} == {v[1] for v in R.CV_WIDE.values()}
    assert {n for (n, p, K, w) in R.SINGLE_DENSE.values() if w} == {65, 257} == {v[0] for v in R.CV_WIDE.values()}
    assert R.wide_leading_dim(208) == 208 and R.wide_leading_dim(209) - 209 == 15 and R.wide_leading_dim(1025) - 1025 == 15
    assert {max(v[2], 1) for v in dense.values()} >= {1, 2, 3, 17, 257} and R.mcov_max_features(3) == 193 and R.mcov_max_features(1) == 198
    # 257 rows of one fit are chunks of 192 and 65; at n = 1025 a chunk is 256 rows: a group of exactly one chunk, one of three
    assert R.rows_per_chunk(257, 33, False) == 192 and R.rows_per_chunk(256, 32, False) == 256 and R.rows_per_chunk(1025, 33, False) == 256
    c = R.cv_dense_case("n1025_Pa33")
    sizes = np.bincount(c.fold)
    assert sizes[0] == 256 and sizes[1] > 2 * 256 and len(set(sizes)) == 3
    assert 1 in np.bincount(R.cv_dense_case("n256_Pa31").fold)
    assert {v[3] for v in dense.values()} >= {1, 3, 10} and R.loo_case().G == 37
    assert {(v[6], v[7]) for v in list(dense.values()) + list(R.CV_WIDE.values())} == {(True, True), (True, False), (False, False)}
    assert {v[5] for v in dense.values()} == {True, False} and {v[4] for v in dense.values() if isinstance(v[4], str)} == {"random", "sorted"}
    # the sparse columns: empty, full, one entry, more than 256 entries, equal and disjoint supports, stored zeros, the two
    # columns of mean 1e6, one with no entry in group 1, one in group 2 only
    s = R.cv_sparse_case("s600")
    nnz = s.stored.sum(axis=0)
    assert nnz[0] == 0 and nnz[1] == 600 and nnz[2] == 1 and nnz[3] > 256 and np.array_equal(s.stored[:, 4], s.stored[:, 5])
    assert not np.any(s.stored[:, 6] & s.stored[:, 7]) and np.any(s.stored[:, 8] & (s.xd[:, 8] == 0)) and nnz[9] == 600 and nnz[10] < 600
    assert abs(s.xd[:, 9].mean() - 1e6) < 1 and not np.any(s.stored[s.fold == 1, 11]) and not np.any(s.stored[s.fold != 2, 12]) and nnz[12] > 0
    d = R.cv_sparse_case("s600", descending=True).x
    assert np.all(np.diff(d.indices[d.indptr[1]:d.indptr[2]]) < 0)
    # the degenerate columns are constant on a training set and not on the data
    for rest in (False, True):
        g = R.degenerate_case(rest, True)
        flags = np.array([R.exactly_constant(g, t) for t in range(g.G)])
        assert flags[:, [1, 3]].any() and flags[:, 6 + 1].any() and not np.all(g.xd[:, 1] == g.xd[0, 1]) and not np.all(g.Y[:, 1] == g.Y[0, 1])
    loo = R.loo_case()
    assert R.exactly_constant(loo, 5)[2] and not R.exactly_constant(loo, 4)[2]


def host_test_inputs():
    """every (x, y, folds, train_on, centre) the pooling restatements of tests/test_cv_covariance_host.py,
    test_cv_mcovariance_host.py, test_cv_wcovariance_host.py and test_cv_wmcovariance_host.py run on, built from those modules'
    own SHAPES, problem() and fold helpers.  standardize and standardize_response do not enter the rule, so each (centre) is
    taken once.  Left out: the 4531-feature shape of cv_wcovariance_reference.SHAPES (three 4533 x 4533 matrices per
    setting)."""
    import cv_wcovariance_reference as crw
    import cv_wmcovariance_reference as crm
    import test_cv_covariance_host as H
    import test_cv_mcovariance_host as HM

    def cases(tag, x, y, fold, G, rests=(False, True), centres=(True, False)):
        for rest in rests:
            if rest and G < 2:
                continue
            for centre in centres:
                yield R.make_case(f"{tag} {x.shape} G={G}", x, y, fold=fold, G=G, rest=rest, centre=centre, standardize=centre)

    for n, p, G in H.SHAPES:                                   # test_cv_covariance_host.py
        x, y = H.problem(n, p)
        for fold in (H.random_folds(n, G), H.sorted_folds(x, G)):
            yield from cases("covariance_host", x, y, fold, G)
    x, y = H.problem(195, 15, seed=1)
    x[:, 3] = 1e6 + np.random.default_rng(5).standard_normal(195)
    for fold in (H.random_folds(195, 3), H.sorted_folds(x[:, [3]], 3)):
        yield from cases("covariance_host mean 1e6", x, y, fold, 3, centres=(True,))
    for n, p, K, G in HM.SHAPES:                               # test_cv_mcovariance_host.py
        x, y = HM.problem(n, p, K)
        for fold in (HM.random_folds(n, G), HM.sorted_folds(x, G)):
            yield from cases("mcovariance_host", x, y, fold, G)
    x, y = HM.problem(195, 13, 5, seed=1)
    x[:, 3] = 1e6 + np.random.default_rng(5).standard_normal(195)
    for fold in (HM.random_folds(195, 3), HM.sorted_folds(x[:, [3]], 3)):
        yield from cases("mcovariance_host mean 1e6", x, y, fold, 3, centres=(True,))
    for n, p, G in crw.SHAPES + [crw.MANY_JOBS]:               # test_cv_wcovariance_host.py
        if p is None:
            continue
        x, y = H.problem(n, p)
        many = (n, p, G) == crw.MANY_JOBS
        yield from cases("wcovariance_host", x, y, H.random_folds(n, G), G, rests=(True,) if many else (False, True),
                         centres=(True, False) if p <= 208 else (True,))
    for n, p, K, G in crm.SMALL_SHAPES:                        # test_cv_wmcovariance_host.py
        yield from cases("wmcovariance_host", *crm.problem(n, p, K, False), crm.equal_folds(n, G) - 1, G)
        x, y = crm.problem(n, p, K, False, seed=3)
        yield from cases("wmcovariance_host sorted", x, y, crm.sorted_folds(x, G), G)
        if p > 2:
            yield from cases("wmcovariance_host mean 1e6", *crm.large_mean_problem(n, p, K, False), crm.equal_folds(n, G, seed=6) - 1, G,
                             centres=(True,))


def test_constant_rule_covers_the_constants_and_nothing_else():
    """on every input of this module (restated as the kernels sum) and on every input of the four host modules (moments by a
    float64 matrix product: constant_margin reads nothing but mu, Mg and total)"""
    own = host = np.inf
    for k in sorted(CV):
        case = CV[k]()
        o = R.product_moments_f64(case) if case.name in BIG else R.restate_cv(case, SUMS["strided256"])
        own = min(own, R.constant_margin(o, case))
    count = 0
    for case in host_test_inputs():
        host = min(host, R.constant_margin(R.product_moments_f64(case), case))
        count += 1
    print(f"constant rule: smallest q / tol over the columns that are not constant on their training set: {own:.3e} on this module's "
          f"{len(CV)} inputs, {host:.3e} on the {count} inputs of tests/test_cv_*_host.py")
    assert own > R.MARGIN and host > R.MARGIN and count > 100
