"""The stages of a cross-validation in the covariance family (sgdnet_amd/csrc/covariance.hip: covariance_cv_run,
mcovariance_cv_run, wcovariance_cv_run, wmcovariance_cv_run) one by one, through sgdnet_cv_covariance_probe, against exact
references (tests/covariance_passes_reference.py).

The end-to-end tests hold a fold fit to KKT <= 1e-8 lambda and to 1e-9 of the separate fit: a pass that loses six digits, an
entry no optimum reads (pairs of coordinates that never become active, the response block, the zero pad of the wide layout),
the bit-for-bit symmetry the wide assembly relies on and the per-training-set outputs are invisible there.  Here every stage is
held to a reference formed from what the stage before it RETURNED; no tolerance was taken from a device run, and
tests/test_covariance_passes_reference.py shows on the CPU that float64 restatements in three summation orders pass these very
checks on these very inputs while eighteen wrong versions do not.

  bitwise   the group matrices symmetric, their corners n_g, a group's matrix whatever the other groups' rows hold, the x-by-x
            block of G = 1 against one fit's; n_T, ridge, the penalties, mean == 0 where not centred, scale == 1 without
            standardize; the wide stats kernel's s and d; S_T symmetric, its pad exactly 0, diag S_T; the wide S_T and c~_T
            against the narrow assembly's Mt / n_T / (f f') at shapes both take; descending rows against ascending; a second call
  bounded   the means, every entry of every group matrix (sparse: over the terms of the kernel's identity), total, and the
            assembly's scale, mean, sd_y / ysd, yy, nulldev, Mt or S_T and c~_T -- against the returned moments, and against
            the long-double moments of x[T], y[T] formed directly, inside the bound of the whole chain (dense and sparse x)
  constant  columns and responses constant on a training set but not on the data: scale exactly 1, exact zeros
The wide feature limit (4531) is not here: its matrix is 164 MB and its long-double truth takes minutes.  Neither is 257 x 1025:
the truth of 65 x 1025 already takes seven seconds.  Each check prints the value closest to its bound (run with -s)."""
import numpy as np
import pytest

import covariance_passes_reference as R

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def probe():
    import torch  # noqa: F401  -- before libsgdnet_hip.so (sgdnet_amd/_lib.py)
    import sgdnet_amd
    L = sgdnet_amd.load()
    if L.sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    assert L.sgdnet_covariance_max_features() == R.COV_MAX_FEATURES and L.sgdnet_mcovariance_max_features(3) == R.mcov_max_features(3)
    from sgdnet_amd import diagnostics
    return diagnostics


def run(probe, case, **kw):
    intercept, standardize = case.centre, case.standardize          # centre = intercept or standardize
    args = dict(train_on="rest" if case.rest else "fold", wide=case.wide, intercept=intercept, standardize=standardize,
                standardize_response=case.standardize_response)
    args.update(kw)
    return probe.cv_covariance_probe(case.x, case.y, case.fold, case.G, case.mixes, case.lam, **args)


@pytest.mark.parametrize("name", list(R.CV_DENSE) + list(R.CV_WIDE))
def test_dense(probe, name):
    case = R.cv_dense_case(name)
    R.check_cv(run(probe, case), case)


@pytest.mark.parametrize("name", ["n63_Pa15", "n256_Pa31", "n1025_Pa33"])
def test_the_wide_assembly_is_the_narrow_one_bit_for_bit(probe, name):
    """at shapes both forms accept: the wide row chunks are other chunks (another any-order sum), so the wide assembly is
    compared with the narrow expressions on ITS OWN moments -- and, where the chunks agree, with the narrow probe's outputs"""
    wide, narrow = R.cv_dense_case(name, wide=True), R.cv_dense_case(name, wide=False)
    ow, on = run(probe, wide), run(probe, narrow)
    R.check_cv(ow, wide)
    if R.rows_per_chunk(wide.n, wide.p + wide.K + 1, True) == R.rows_per_chunk(wide.n, wide.p + wide.K + 1, False):
        assert np.array_equal(ow.Mg, on.Mg)
        R.check_wide_equals_narrow(ow, on, wide)
    # the narrow expressions in float64 on the wide run's own returned moments
    R.check_wide_equals_narrow(ow, R.restate_cv(narrow, given=ow), wide)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("name", list(R.CV_SPARSE))
def test_sparse(probe, name, wide):
    case = R.cv_sparse_case(name, wide=wide)
    R.check_cv(run(probe, case), case)


@pytest.mark.parametrize("name", ["s600", "s257_K2"])
def test_descending_rows_give_the_bits_of_ascending_rows(probe, name):
    R.same_bits(run(probe, R.cv_sparse_case(name, descending=True)), run(probe, R.cv_sparse_case(name)), name)


@pytest.mark.parametrize("wide", [False, True])
def test_a_matrix_that_stores_nothing(probe, wide):
    case = R.empty_sparse_cv_case(wide)
    o = run(probe, case)
    R.check_cv(o, case)
    assert np.all(o.scale == 1.0) and np.all(o.Mg[:, :case.p, :] == 0.0)


@pytest.mark.parametrize("wide", [False, True])
def test_leave_one_out_and_its_one_hot_column(probe, wide):
    case = R.loo_case(wide)
    o = run(probe, case)
    R.check_cv(o, case)
    assert R.exactly_constant(case, 5)[2] and o.scale[5, 2] == 1.0
    assert R.constant_margin(o, case) > R.MARGIN


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("rest", [False, True])
def test_columns_constant_on_a_training_set(probe, rest, multi, wide):
    """the indicator that is all 0 on T, the integer-valued column constant on T, the response constant on T: scale (and
    ysd) exactly 1, row and column of what the path kernel reads and c~ exactly 0, no contribution to yy and nulldev"""
    case = R.degenerate_case(rest, multi, wide)
    o = run(probe, case)
    R.check_cv(o, case)
    assert R.constant_margin(o, case) > R.MARGIN
    for t in range(case.G):
        const = R.exactly_constant(case, t)
        cx = const[:case.p]
        assert np.all(o.scale[t][cx] == 1.0)
        if wide:
            assert np.all(o.S[t][cx] == 0.0) and np.all(o.S[t][:, :case.p][:, cx] == 0.0) and np.all(o.ct[t][cx] == 0.0)
        else:
            assert np.all(o.Mt[t][:case.p][cx] == 0.0) and np.all(o.Mt[t][:, :case.p][:, cx] == 0.0)


def test_constant_columns_without_standardize(probe):
    case = R.degenerate_case(False, True, False, standardize=False, standardize_response=False)
    R.check_cv(run(probe, case), case)


@pytest.mark.parametrize("wide", [False, True])
def test_a_response_constant_on_a_training_set(probe, wide):
    case = R.constant_response_case(wide)
    o = run(probe, case)
    R.check_cv(o, case)
    assert o.tstat[1, 1] == 1.0 and o.tstat[2, 1] == 0.0 and np.all((o.ct[1] if wide else o.Mt[1][:, case.p]) == 0.0)


def _two_rows_of_group_2(case):
    rows = np.flatnonzero(case.fold == 2)
    return int(rows[3]), int(rows[4])


def test_a_group_does_not_see_another_groups_rows(probe):
    """rows of group 2 change: the matrices of groups 0 and 1 keep their bits, group 2's does not.  Uncentred, the common
    centre is 0 whatever the rows hold.  Centred, the centre is the whole-data mean, which every row enters: x holds small
    integers (every column sum exact in any order) and two rows of group 2 move by +1 and -1, so the sums, and with them
    the centres, keep their bits."""
    case = R.cv_dense_case("n1025_Pa33")
    i, j = _two_rows_of_group_2(case)
    x = case.x.copy()
    x[i] = x[i] + 0.5
    kw = dict(fold=case.fold, G=case.G, rest=False, centre=False, standardize=False)
    a, b = run(probe, R.make_case("uncentred", case.x, case.y, **kw)), run(probe, R.make_case("uncentred_changed", x, case.y, **kw))
    assert np.array_equal(a.mu, b.mu) and np.array_equal(a.Mg[:2], b.Mg[:2]) and not np.array_equal(a.Mg[2], b.Mg[2])
    xi = np.random.default_rng(12).integers(-8, 9, case.x.shape).astype(np.float64)
    xc = xi.copy()
    xc[i] += 1.0
    xc[j] -= 1.0
    kw = dict(fold=case.fold, G=case.G, rest=True, centre=True, standardize=True)
    a, b = run(probe, R.make_case("integers", xi, case.y, **kw)), run(probe, R.make_case("integers_changed", xc, case.y, **kw))
    assert np.any(a.mu[:case.p] != 0.0) and np.array_equal(a.mu, b.mu)
    assert np.array_equal(a.Mg[:2], b.Mg[:2]) and not np.array_equal(a.Mg[2], b.Mg[2])


def test_one_group_is_the_single_fit_bit_for_bit(probe):
    """with G = 1 the x-by-x block of Mg[0] is one fit's M block: the same centres, tiles and chunks (the code promises this)"""
    case = R.cv_dense_case("n257_Pa32_G1")
    o = run(probe, case)
    single = probe.covariance_probe(case.x, case.y - case.y.mean(axis=0), np.ones(case.p), 0.5, [0.1])
    p = case.p
    assert np.array_equal(single.mu[:p], o.mu[:p]) and np.array_equal(single.M[:p, :p], o.Mg[0][:p, :p])


@pytest.mark.parametrize("name,wide", [("n256_Pa31", False), ("n63_Pa15", True)])
def test_a_second_call_returns_the_same_bits(probe, name, wide):
    case = R.cv_dense_case(name, wide=wide)
    R.same_bits(run(probe, case), run(probe, case), name)


def test_the_probe_refuses_what_the_fit_refuses(probe):
    from sgdnet_amd import SgdnetError
    import sgdnet_amd as sa

    def refusal(code, needle, case, **kw):
        with pytest.raises(SgdnetError) as e:
            run(probe, case, **kw)
        assert e.value.code == code and needle in str(e.value), (code, needle, str(e.value))
        return str(e.value)

    rng = np.random.default_rng(0)
    ok = R.cv_dense_case("n63_Pa15")
    wide_x = rng.standard_normal((20, R.COV_MAX_FEATURES + 1))
    too_wide = R.make_case("p199", wide_x, rng.standard_normal(20), fold=np.arange(20) % 2, G=2)
    words = refusal(EUNSUPPORTED, "mode = covariance needs no more features than sgdnet_covariance_max_features()", too_wide)
    with pytest.raises(SgdnetError) as e:        # the fit's own words, letter for letter
        sa.cv_covariance_fits(wide_x, too_wide.y, too_wide.fold, 0.5, [0.1, 0.01])
    assert str(e.value) == words and e.value.code == EUNSUPPORTED
    refusal(EUNSUPPORTED, "mode = covariance needs one GPU", ok, n_gpus=2)
    refusal(EUNSUPPORTED, "mode = covariance needs debug = 0", ok, debug=1)
    refusal(EUNSUPPORTED, "mode = wcovariance needs family = gaussian", ok, wide=True, family="binomial")
    refusal(EUNSUPPORTED, "mode = mcovariance needs at least two responses", ok, family="mgaussian", n_classes=1)
    bad = R.make_case("bad_fold", ok.x, ok.y, fold=np.where(np.arange(ok.n) == 7, 3, ok.fold), G=3)
    refusal(EINVAL, "fold[7] = 3 is not a group id in 0..2", bad)
    empty = R.make_case("empty_group", ok.x, ok.y, fold=np.minimum(ok.fold, 1), G=3)
    refusal(EINVAL, "group 2 of 3 is empty", empty)
    one = R.make_case("one_group", ok.x, ok.y, fold=np.zeros(ok.n), G=1, rest=True)
    refusal(EINVAL, "train_on_rest needs two groups", one)
    neg = R.make_case("negative_lambda", ok.x, ok.y, fold=ok.fold, G=3, lam=(0.1, -0.01))
    refusal(EINVAL, "is negative", neg)
    mix = R.make_case("bad_mix", ok.x, ok.y, fold=ok.fold, G=3, mixes=(0.5, 1.5))
    refusal(EINVAL, "is not an elastic-net mix", mix)
