"""CPU proof that the bounds of tests/newton_reference.py admit any legal summation order and reject wrong formulas, on
the very inputs tests/test_gpu_newton_passes.py gives the device: one outer step of Newton mode is carried out in float64
(newton_reference.restate) with the sums taken sequentially, pairwise, and in the 256-thread strided-then-tree order of
block_sum, and every pass must stay inside its bound around the long-double truth (newton_reference.check_probe, the
checks the GPU test applies to the device's outputs).  Then seven wrong formulas, each of which must fall outside the
bound of its pass on a named input."""
import os

import numpy as np
import pytest

import newton_reference as R

MIX = dict((name, (l2, l1, ridge)) for name, l2, l1, ridge in R.PENALTIES)


def _step(case, kind, pen="mix0.5", fsum=R.seq_sum, wrong=None, **kw):
    l2, l1, ridge = MIX[pen]
    u = R.candidate(case, kind)
    o = R.restate(case, u, 0.5, l2, l1, ridge, fsum=fsum, wrong=wrong, **kw)
    return o, u, (l2, l1, ridge)


def _check_every_order(case, kinds, pens):
    for kind, pen in zip(kinds, pens):
        for fsum in R.SUMS.values():
            o, u, (l2, l1, ridge) = _step(case, kind, pen, fsum)
            R.check_probe(o, case, u, 0.5, l2, l1, ridge)


PENS = [name for name, *_ in R.PENALTIES]


@pytest.mark.parametrize("centre", [0, 1])
@pytest.mark.parametrize("n,p", R.DENSE_SHAPES)
def test_dense_bounds_admit_every_summation_order(n, p, centre):
    kinds = list(R.CANDIDATES) if p is not None else ["moderate", "overflow"]
    _check_every_order(R.dense_case(n, p, centre), kinds, (PENS + PENS)[:len(kinds)])


@pytest.mark.parametrize("centre", [0, 1])
@pytest.mark.parametrize("n", R.SPARSE_N)
def test_sparse_bounds_admit_every_summation_order(n, centre):
    _check_every_order(R.sparse_case(n, centre, descending=(n == 257)), list(R.CANDIDATES), PENS + PENS)


def test_empty_sparse_bounds():
    for centre in (0, 1):
        _check_every_order(R.empty_sparse_case(255, 3, centre), ["zero", "moderate"], PENS)


def test_one_sweep_and_a_frozen_intercept_stay_inside():
    case = R.dense_case(65, 16, 1)
    for fit_intercept in (True, False):
        o, u, (l2, l1, ridge) = _step(case, "moderate", "mix0.5", max_sweeps=1, fit_intercept=fit_intercept)
        assert o.cd_rec["sweeps"] == 1.0
        R.check_probe(o, case, u, 0.5, l2, l1, ridge, fit_intercept=fit_intercept, max_sweeps=1)


def test_the_sparse_identity_is_the_centred_sum():
    """with V and R the exact sums, the identity the sparse truth evaluates IS sum_i w_i d_ij d_ik over all rows"""
    case = R.sparse_case(255, 1)
    o, _u, _ = _step(case, "moderate")
    V, R_ = np.asarray(o.v, dtype=R.LD).sum(), np.asarray(o.r, dtype=R.LD).sum()
    ident = R.sparse_moment_reference(case.xd, case.stored, o.mean, o.v, o.r, V, R_)
    T = R.centred_moment_truth(case.xd, o.mean, o.v, o.r)
    k = R.upper(case.p + 2)
    # the long-double evaluation of the identity cancels like the kernel's: 2^-11 of the float64 bound covers it
    assert np.all(np.abs(ident.v - T)[k] <= ident.e[k] / 2048 + 1e-30)


def test_bounds_are_rounding_bounds_not_tolerances():
    case = R.dense_case(257, 30, 1)
    o, u, _ = _step(case, "wide")
    s = R.state_reference(case.xd, o.mean, o.pub_a, case.y)
    assert float(s.v.e.max()) < 1e-13 and float(s.r.e.max()) < 1e-13          # absolute, about u of 1
    m = R.dense_moment_reference(case.xd, o.mean, o.v, o.r)
    k = R.upper(case.p + 2)
    T = R.centred_moment_truth(case.xd, o.mean, o.v, o.r)
    assert np.all(np.abs(m.v - T)[k] <= 1e-15 * np.abs(T[k]).max())
    assert float(m.e[k].max()) < 1e-12 * float(np.abs(T[k]).max())


# (wrong formula, the input it must show on, the pass whose check must fail)
WRONG = [("v_is_t_squared", ("dense", 63, 14), "state: v"),
         ("neither_dropped", ("sparse", 255), "moments: M"),
         ("only_k_unweighted", ("sparse", 255), "moments: M"),
         ("full_shortcut_always", ("sparse", 255), "moments: M"),
         ("V_for_R", ("sparse", 255), "moments: M"),
         ("no_1_over_n", ("dense", 63, 14), "inner:"),
         ("q_staged_as_vr", ("dense", 63, 14), "moments: M")]


@pytest.mark.parametrize("wrong,where,fails", WRONG)
def test_wrong_formulas_fall_outside(wrong, where, fails):
    case = R.dense_case(where[1], where[2], 1) if where[0] == "dense" else R.sparse_case(where[1], 1)
    o, u, (l2, l1, ridge) = _step(case, "moderate", wrong=wrong)
    with pytest.raises(AssertionError, match=fails):
        R.check_probe(o, case, u, 0.5, l2, l1, ridge)
    o, u, _ = _step(case, "moderate")
    R.check_probe(o, case, u, 0.5, l2, l1, ridge)            # the right formula on the same input stays inside


def test_one_over_n_shows_in_a_single_sweep_too():
    case = R.dense_case(63, 14, 1)
    l2, l1, ridge = MIX["mix0.5"]
    u = R.candidate(case, "moderate")
    o = R.restate(case, u, 0.5, l2, l1, ridge, max_sweeps=1, wrong="no_1_over_n")
    with pytest.raises(AssertionError, match="inner: single sweep"):
        R.check_inner(o, case, l2, l1, ridge, True, 1, 1e-7)


def test_probe_refusals_and_no_device():
    """the probe refuses by name what the plan refuses, before it looks for a device; without one it says so"""
    import ctypes as C

    import sgdnet_amd as sa
    from sgdnet_amd import _lib, diagnostics
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sgdnet_hip.h")).read()
    assert "int sgdnet_newton_probe_dense(" in hdr and "int sgdnet_newton_probe_sparse(" in hdr and _lib.ABI_VERSION == 6
    assert R.MAX_FEATURES == sa.newton_max_features()
    l2, l1, ridge = MIX["mix0.5"]
    wide = R.dense_case(20, R.MAX_FEATURES + 1, 1)
    with pytest.raises(sa.SgdnetError, match=r"mode = newton needs no more features than sgdnet_newton_max_features\(\)") as e:
        diagnostics.newton_probe(wide.x, wide.y, wide.scale, wide.u_cur, wide.u_cur)
    assert e.value.code == -5
    case = R.dense_case(20, 3, 1)
    with pytest.raises(sa.SgdnetError, match="sgdnet_newton_probe_dense: invalid argument") as e:
        diagnostics.newton_probe(case.x, case.y, case.scale, case.u_cur, case.u_cur, max_sweeps=0)
    assert e.value.code == -1
    L = sa.load()
    pr = _lib.NewtonProbe()                               # every pointer NULL
    assert L.sgdnet_newton_probe_dense(_lib.dptr(np.asfortranarray(case.x)), 20, 3, 0, C.byref(pr)) == -1
    assert L.sgdnet_newton_probe_dense(None, 20, 3, 0, C.byref(pr)) == -1 and b"invalid matrix" in L.sgdnet_last_error()
    assert L.sgdnet_newton_probe_sparse(None, 0, C.byref(pr)) == -1 and b"invalid matrix" in L.sgdnet_last_error()
    sc = R.sparse_case(20, 1)
    with pytest.raises(sa.SgdnetError, match="sgdnet_newton_probe_sparse: invalid argument"):
        diagnostics.newton_probe(sc.x, sc.y, sc.scale, sc.u_cur, sc.u_cur, max_sweeps=0)
    if L.sgdnet_device_count() == 0:
        for c in (case, sc):
            with pytest.raises(sa.SgdnetError, match="no HIP device") as e:
                diagnostics.newton_probe(c.x, c.y, c.scale, c.u_cur, c.u_cur)
            assert e.value.code == -2
