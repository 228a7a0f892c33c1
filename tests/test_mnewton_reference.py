"""CPU proof that the bounds of tests/mnewton_reference.py admit any legal summation order and reject wrong formulas, on the
very inputs tests/test_gpu_mnewton_passes.py gives the device: one outer step of multinomial Newton mode is carried out in
float64 (mnewton_reference.restate) with the any-order sums taken sequentially, pairwise, and in the 256-thread
strided-then-tree order of block_sum, and every pass must stay inside its bound around the long-double truth
(mnewton_reference.check_probe, the checks the GPU test applies to the device's outputs).  Every case the GPU test holds
to optimality converges here within the kernel's cap of 1000 sweeps.  Then ten wrong formulas, each of which must fall
outside the bound of its pass on a named input."""
import os

import numpy as np
import pytest

import mnewton_reference as R

MIX = dict((name, (l2, l1, ridge)) for name, l2, l1, ridge in R.PENALTIES)
ORDERS = list(R.SUMS.values())


def _step(case, kind, pen="mix0.5", fsum=R.seq_sum, wrong=None, t=0.5, **kw):
    l2, l1, ridge = MIX[pen]
    u = R.candidate(case, kind)
    o = R.restate(case, u, t, l2, l1, ridge, fsum=fsum, wrong=wrong, **kw)
    return o, u, (l2, l1, ridge)


def _check(case, kind, pen, fsums):
    plan = R.solve_plan(case, kind, pen)
    for fsum in fsums:
        o, u, (l2, l1, ridge) = _step(case, kind, pen, fsum, max_sweeps=plan["max_sweeps"])
        R.check_probe(o, case, u, 0.5, l2, l1, ridge, **plan)


def _by_shape(runs):
    shapes = []
    for n, p, K, centre, _kind, _pen in runs:
        if (n, p, K, centre) not in shapes:
            shapes.append((n, p, K, centre))
    return shapes


EDGE_RUNS = R.runs(R.EDGE_SHAPES)
LIMIT_RUNS = R.runs(R.LIMIT_SHAPES, kinds=("moderate", "wide", "overflow"), centres=(1,))


@pytest.mark.parametrize("n,p,K,centre", _by_shape(EDGE_RUNS))
def test_bounds_admit_every_summation_order(n, p, K, centre):
    """every order on the small shapes; from 600 rows on the orders take turns over the candidates"""
    case = R.case(n, p, K, centre)
    for i, (_n, _p, _K, _c, kind, pen) in enumerate(r for r in EDGE_RUNS if r[:4] == (n, p, K, centre)):
        _check(case, kind, pen, ORDERS if n < 600 else [ORDERS[i % 3]])


@pytest.mark.parametrize("n,p,K,centre", _by_shape(LIMIT_RUNS))
def test_bounds_at_the_limits(n, p, K, centre):
    case = R.case(n, p, K, centre)
    for i, (_n, _p, _K, _c, kind, pen) in enumerate(r for r in LIMIT_RUNS if r[:4] == (n, p, K, centre)):
        _check(case, kind, pen, [ORDERS[i % 3]])


@pytest.mark.parametrize("pen", list(MIX))
@pytest.mark.parametrize("n,p,K", R.STRIDE_SHAPES)
def test_stride_shapes_with_and_without_the_intercept_and_one_sweep(n, p, K, pen):
    case = R.case(n, p, K, 1)
    l2, l1, ridge = MIX[pen]
    for kw in (dict(must_converge=True), dict(fit_intercept=False, must_converge=True), dict(max_sweeps=1)):
        run = {k: v for k, v in kw.items() if k != "must_converge"}
        o, u, _ = _step(case, "moderate", pen, **run)
        R.check_probe(o, case, u, 0.5, l2, l1, ridge, **kw)
        if kw.get("fit_intercept") is False:
            b = np.arange(case.Q) % case.P == case.p
            assert np.array_equal(o.cd_u[b], case.u_cur[b])


def test_a_class_without_a_member_and_the_degenerate_inputs_stay_inside():
    case = R.case(65, 15, 3, 1, empty_class=1)
    assert not np.any(case.y == 1)
    _check(case, "moderate", "mix0.5", ORDERS)
    case = R.case(65, 15, 3, 1)
    case.xd[:, 2] = 3.0
    for pen in ("mix1", "mix0.5"):
        o, u, (l2, l1, ridge) = _step(case, "moderate", pen)
        R.check_probe(o, case, u, 0.5, l2, l1, ridge, must_converge=True)
        j = np.arange(case.K) * case.P + 2
        assert np.all(o.cd_u[j] == 0.0) if l2 > 0 else np.array_equal(o.cd_u[j], case.u_cur[j])
    u = np.zeros(case.Q)
    u[case.p] = 800.0
    for pen in ("mix0.5", "mix1"):
        l2, l1, ridge = MIX[pen]
        o = R.restate(case, u, 0.5, l2, l1, ridge)
        R.check_probe(o, case, u, 0.5, l2, l1, ridge)
        assert np.all(o.mu[:, 0] == 1.0) and np.all(o.mu[:, 1:] == 0.0) and np.isfinite(o.loss)


def test_every_case_held_to_optimality_converges():
    """the float64 restatement of the inner solve on the project's own cases: converged within the cap wherever
    mnewton_reference.converges says so (the GPU test asserts the device's flag on exactly these)"""
    worst = 0
    for n, p, K, centre, kind, pen in EDGE_RUNS + LIMIT_RUNS + R.runs(R.STRIDE_SHAPES, kinds=("moderate",), centres=(1,)):
        case = R.case(n, p, K, centre)
        if not R.converges(case, kind, pen):
            continue
        o, _u, _ = _step(case, kind, pen)
        assert o.cd_rec["converged"] == 1.0, (n, p, K, centre, kind, pen, o.cd_rec)
        worst = max(worst, int(o.cd_rec["sweeps"]))
    print("most sweeps:", worst)
    assert worst < 1000


def test_bounds_are_rounding_bounds_not_tolerances():
    """a relative perturbation of 1e-12 of any output falls outside its bound"""
    case = R.case(63, 13, 3, 1)
    l2, l1, ridge = MIX["mix0.5"]
    u = R.candidate(case, "moderate")

    def fresh():
        return R.restate(case, u, 0.3, l2, l1, ridge)

    R.check_probe(fresh(), case, u, 0.3, l2, l1, ridge, must_converge=True)
    eps = 1 + 1e-12
    for name, fails in (("mean", "mean"), ("mu", "state: mu"), ("M", "moments: M"), ("blend_u", "blend: u"), ("pub_a", "publish: a"),
                        ("cd_a", "inner: a")):
        o = fresh()
        setattr(o, name, getattr(o, name) * eps)
        with pytest.raises(AssertionError, match=fails):
            R.check_probe(o, case, u, 0.3, l2, l1, ridge)
    for rec, key, fails in (("pub_rec", "half_sq", "publish: half_sq"), ("blend_rec", "abs", "blend: abs"), ("cd_rec", "half_sq", "inner: half_sq"),
                            ("cd_rec", "size", "inner: change / size")):
        o = fresh()
        getattr(o, rec)[key] *= eps
        with pytest.raises(AssertionError, match=fails):
            R.check_probe(o, case, u, 0.3, l2, l1, ridge)
    o = fresh()
    o.loss *= eps
    with pytest.raises(AssertionError, match="state: loss"):
        R.check_probe(o, case, u, 0.3, l2, l1, ridge)
    # the single sweep: the candidate itself
    o = R.restate(case, u, 0.3, l2, l1, ridge, max_sweeps=1)
    R.check_inner(o, case, l2, l1, ridge, True, 1, 1e-7)
    o.cd_u = o.cd_u * eps
    o.cd_a = np.where(R.penalised(case.K, case.p), o.cd_u / np.tile(np.concatenate([case.scale, [1.0]]), case.K), o.cd_u)
    h, a = R.record_f64(o.cd_u, case.K, R.seq_sum)
    o.cd_rec.update(half_sq=h, abs=a, size=float(np.abs(o.cd_u).max()), change=float(np.abs(o.cd_u - case.u_cur).max()))
    with pytest.raises(AssertionError, match="inner: single sweep"):
        R.check_inner(o, case, l2, l1, ridge, True, 1, 1e-7)


# (wrong formula, (n, p, K), candidate, the check that must fail)
WRONG = [("offdiag_plus", (63, 13, 3), "moderate", "moments: M"),
         ("block_diagonal", (63, 13, 3), "moderate", "inner:"),
         ("pairs_swapped", (63, 13, 3), "moderate", "moments: M"),
         ("q_on_offdiag", (63, 13, 3), "moderate", "moments: M: the q column of the off-diagonal pair"),
         ("q_uses_mu_l", (63, 13, 3), "moderate", "moments: M"),
         ("no_max", (65, 15, 3), "overflow", "state:"),
         ("no_1_over_n", (63, 13, 3), "moderate", "inner:"),
         ("scale_by_joint_index", (63, 13, 3), "moderate", "inner:"),
         ("penalty_with_intercepts", (63, 13, 3), "moderate", "publish: half_sq"),
         ("loss_eta_0", (63, 13, 3), "moderate", "state: loss")]


@pytest.mark.parametrize("wrong,shape,kind,fails", WRONG)
def test_wrong_formulas_fall_outside(wrong, shape, kind, fails):
    case = R.case(*shape, 1)
    plan = R.solve_plan(case, kind, "mix0.5")
    o, u, (l2, l1, ridge) = _step(case, kind, wrong=wrong, max_sweeps=plan["max_sweeps"])
    with pytest.raises(AssertionError, match=fails):
        R.check_probe(o, case, u, 0.5, l2, l1, ridge, **plan)
    o, u, _ = _step(case, kind, max_sweeps=plan["max_sweeps"])
    R.check_probe(o, case, u, 0.5, l2, l1, ridge, **plan)            # the right formula on the same input stays inside


@pytest.mark.parametrize("wrong", ["block_diagonal", "no_1_over_n", "scale_by_joint_index"])
def test_wrong_curvature_shows_in_a_single_sweep_too(wrong):
    case = R.case(63, 13, 3, 1)
    l2, l1, ridge = MIX["mix0.5"]
    u = R.candidate(case, "moderate")
    o = R.restate(case, u, 0.5, l2, l1, ridge, max_sweeps=1, wrong=wrong)
    with pytest.raises(AssertionError, match="inner: single sweep"):
        R.check_inner(o, case, l2, l1, ridge, True, 1, 1e-7)


def test_probe_refusals_and_no_device():
    """the probe refuses by name what the plan refuses, before it looks for a device; without one it says so"""
    import ctypes as C

    import sgdnet_amd as sa
    from sgdnet_amd import _lib, diagnostics
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sgdnet_hip.h")).read()
    assert "int sgdnet_mnewton_probe(" in hdr and _lib.ABI_VERSION == 6
    for K, limit in R.MAX_FEATURES.items():
        assert sa.mnewton_max_features(K) == limit
    for K in (2, 3, 10, 99, 100):
        limit = sa.mnewton_max_features(K)
        wide = R.case(20, limit + 1, K, 1)
        with pytest.raises(sa.SgdnetError, match=r"mode = mnewton needs no more features than sgdnet_mnewton_max_features\(n_classes\)") as e:
            diagnostics.mnewton_probe(wide.x, wide.y, K, wide.scale, wide.u_cur, wide.u_cur)
        assert e.value.code == -5 and "(limit %d)" % limit in str(e.value)
    case = R.case(20, 3, 3, 1)
    for kw in (dict(max_sweeps=0), dict(width=128), dict(width=-64), dict(width=1)):
        with pytest.raises(sa.SgdnetError, match="sgdnet_mnewton_probe: invalid argument") as e:
            diagnostics.mnewton_probe(case.x, case.y, 3, case.scale, case.u_cur, case.u_cur, **kw)
        assert e.value.code == -1
    for K in (1, 0, -3):
        with pytest.raises(sa.SgdnetError, match="sgdnet_mnewton_probe: invalid argument") as e:
            diagnostics.mnewton_probe(case.x, case.y, K, case.scale, case.u_cur[:max(K, 0) * 4], case.u_cur[:max(K, 0) * 4])
        assert e.value.code == -1
    L = sa.load()
    pr = _lib.MNewtonProbe()                              # every pointer NULL
    pr.K, pr.max_sweeps = 3, 10
    xf = np.asfortranarray(case.x)
    assert L.sgdnet_mnewton_probe(_lib.dptr(xf), 20, 3, 0, C.byref(pr)) == -1 and b"invalid argument" in L.sgdnet_last_error()
    assert L.sgdnet_mnewton_probe(_lib.dptr(xf), 20, 3, 0, None) == -1
    for n, p in ((0, 3), (20, 0)):
        assert L.sgdnet_mnewton_probe(_lib.dptr(xf), n, p, 0, C.byref(pr)) == -1 and b"invalid matrix" in L.sgdnet_last_error()
    assert L.sgdnet_mnewton_probe(None, 20, 3, 0, C.byref(pr)) == -1 and b"invalid matrix" in L.sgdnet_last_error()
    if L.sgdnet_device_count() == 0:
        with pytest.raises(sa.SgdnetError, match="no HIP device") as e:
            diagnostics.mnewton_probe(case.x, case.y, 3, case.scale, case.u_cur, case.u_cur)
        assert e.value.code == -2
