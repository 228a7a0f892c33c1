"""CPU proof that the checks of tests/wide_passes_reference.py admit any legal summation order and reject wrong versions, on
the very inputs tests/test_gpu_wnewton_passes.py and tests/test_gpu_wmnewton_passes.py give the device: one outer step of a
wide Newton mode is carried out in float64 (wn_restate / wmn_restate) with the any-order sums taken sequentially, pairwise
and in block_sum's order, and every pass must pass the checks the GPU tests apply to the device's outputs.  Then the wrong
versions (`wrong=` switches of the scale restatements and of list_solve), each of which must fail a named check on a named
input, and the conditions the list cases have to satisfy, asserted from the restatement alone."""
import os

import numpy as np
import pytest

import mnewton_reference as MN
import newton_reference as N
import wide_passes_reference as W

ORDERS = list(W.SUMS.values())
WN_RUNS = W.count_runs(W.WN_COUNTS)
WMN_RUNS = W.count_runs(W.WMN_SHAPES + [W.WMN_MANY_CLASSES])
N_ROWS = 48


def _wn(case, kind, pen=None, fsum=W.seq_sum, wrong=None, t=0.5, **kw):
    if pen is not None:
        l2, l1, ridge = W.MIX[pen]
        kw = dict(kw, l2=l2, l1=l1, ridge=ridge)
    u = N.candidate(case, kind)
    return W.wn_restate(case, u, t, fsum=fsum, wrong=wrong, **kw), u


def _wmn(case, kind, pen=None, fsum=W.seq_sum, wrong=None, t=0.5, **kw):
    if pen is not None:
        l2, l1, ridge = W.MIX[pen]
        kw = dict(kw, l2=l2, l1=l1, ridge=ridge)
    u = MN.candidate(case, kind)
    return W.wmn_restate(case, u, t, fsum=fsum, wrong=wrong, **kw), u


def _held(kw):
    """the arguments of the checks from those of a restatement"""
    return {k: v for k, v in kw.items() if k in ("l2", "l1", "ridge", "fit_intercept", "max_sweeps", "tol")}


@pytest.mark.parametrize("P,centre,kind,pen", WN_RUNS)
def test_wnewton_counts_stay_inside_in_every_order(P, centre, kind, pen):
    """every order up to 257 coordinates; beyond, the orders take turns"""
    case = W.wn_case(N_ROWS, P - 1, centre)
    plan = W.solve_plan(kind, pen, case.n, P)
    l2, l1, ridge = W.MIX[pen]
    for fsum in (ORDERS if P <= 257 else [ORDERS[P % 3]]):
        o, u = _wn(case, kind, pen, fsum, max_sweeps=plan["max_sweeps"])
        W.wn_check_probe(o, case, u, 0.5, l2, l1, ridge, **plan)


@pytest.mark.parametrize("shape,centre,kind,pen", WMN_RUNS)
def test_wmnewton_counts_stay_inside_in_every_order(shape, centre, kind, pen):
    K, p = shape
    case = W.wmn_case(N_ROWS, p, K, centre)
    plan = W.solve_plan(kind, pen, case.n, case.Q)
    l2, l1, ridge = W.MIX[pen]
    for fsum in (ORDERS if case.Q <= 258 else [ORDERS[case.Q % 3]]):
        o, u = _wmn(case, kind, pen, fsum, max_sweeps=plan["max_sweeps"])
        W.wmn_check_probe(o, case, u, 0.5, l2, l1, ridge, **plan)


def test_row_chunk_inputs_stay_inside():
    """the inputs of the GPU tests' row-chunk cases, one order each; at p + 2 = 496 / 497 the moments on the sample"""
    for i, ncols in enumerate((496, 497)):
        case = W.wn_case(257, ncols - 2, 1)
        o, u = _wn(case, "moderate", "mix0.5", ORDERS[i], max_sweeps=1)
        W.wn_check_probe(o, case, u, 0.5, *W.MIX["mix0.5"], max_sweeps=1, sampled=True)
    for i, ncols in enumerate((272, 273)):
        c = W.wmn_case(257, ncols - 2, 2, 1)
        o, u = _wmn(c, "moderate", "mix0.5", ORDERS[i + 1], max_sweeps=1)
        W.wmn_check_probe(o, c, u, 0.5, *W.MIX["mix0.5"], max_sweeps=1, sampled=True)
    for i, n in enumerate((255, 256, 257, 513)):
        case, c = W.wn_case(n, 7, n % 2), W.wmn_case(n, 7, 2, n % 2)
        plan = W.solve_plan("wide", "mix0.5", n, 8)
        o, u = _wn(case, "wide", "mix0.5", ORDERS[i % 3], max_sweeps=plan["max_sweeps"])
        W.wn_check_probe(o, case, u, 0.5, *W.MIX["mix0.5"], **plan)
        o, u = _wmn(c, "wide", "mix0.5", ORDERS[i % 3], max_sweeps=plan["max_sweeps"])
        W.wmn_check_probe(o, c, u, 0.5, *W.MIX["mix0.5"], **plan)


@pytest.mark.parametrize("mode", ["wnewton", "wmnewton"])
def test_the_limit_inputs_stay_inside_and_converge(mode):
    """5820 coordinates: the scale pass in full, the moments on the sample, the list solve converged and optimal"""
    if mode == "wnewton":
        case = W.wn_limit_case()
        o, u = _wn(case, "moderate", **W.LIMIT_PENALTY)
        W.wn_check_probe(o, case, u, 0.5, sampled=True, must_converge=True, **W.LIMIT_PENALTY)
    else:
        case = W.wmn_limit_case()
        o, u = _wmn(case, "moderate", **W.WMN_LIMIT_PENALTY)
        W.wmn_check_probe(o, case, u, 0.5, sampled=True, must_converge=True, **W.WMN_LIMIT_PENALTY)
    print("sweeps", o.solve.sweeps, "screens added", o.solve.added)
    assert o.solve.sweeps < 800


@pytest.mark.parametrize("t", [1.0, 0.5, 0.3])
def test_blend_inputs_stay_inside(t):
    """P = 100 and Q = 99; t = 1 and 0.5 bitwise, 0.3 three roundings"""
    case, c = W.wn_case(N_ROWS, 99, 1), W.wmn_case(N_ROWS, 32, 3, 1)
    l2, l1, ridge = W.MIX["mix0.5"]
    o, u = _wn(case, "moderate", "mix0.5", t=t)
    W.wn_check_probe(o, case, u, t, l2, l1, ridge, must_converge=True)
    o, u = _wmn(c, "moderate", "mix0.5", t=t)
    W.wmn_check_probe(o, c, u, t, l2, l1, ridge, must_converge=True)


def test_narrow_against_wide_inputs_stay_inside_and_converge():
    l2, l1, ridge = W.MIX["mix0.5"]
    for i, p in enumerate((64, 198)):
        case = W.wn_case(300, p, 1)
        o, u = _wn(case, "moderate", "mix0.5", ORDERS[i])
        W.wn_check_probe(o, case, u, 0.5, l2, l1, ridge, must_converge=True)
    for i, (K, p) in enumerate(((3, 21), (3, 65))):
        c = W.wmn_case(300, p, K, 1)
        o, u = _wmn(c, "moderate", "mix0.5", ORDERS[i + 1])
        W.wmn_check_probe(o, c, u, 0.5, l2, l1, ridge, must_converge=True)


def test_the_shapes_sit_where_the_code_branches():
    """read off csrc/wide_layout.hpp, csrc/wide_cd_device.hpp and csrc/mnewton.hpp"""
    assert [W.leading_dim(c) - c for c in (2, 16, 17, 32, 33, 1025)] == [14, 0, 15, 0, 15, 15]
    assert [K * (p + 1) for K, p in W.WMN_SHAPES] == [4, 6, 15, 16, 18, 32, 33, 64, 65, 66, 255, 256, 258, 1023, 1024, 1025, 1026]
    assert W.WMN_MANY_CLASSES[0] * (W.WMN_MANY_CLASSES[1] + 1) == 260
    # the row chunks of the wide moments passes: 31 tiles, 496 pairs, two chunks against 32 tiles, 528 pairs, one chunk
    assert W.wide_row_chunks(257, 496) == 2 and W.wide_row_chunks(257, 497) == 1
    # wmnewton at K = 2 (3 class pairs): 18 tiles, 171 pairs, 513 workgroups, one chunk; 17 tiles, 153 pairs, 459 workgroups, two
    assert W.wide_row_chunks(257, 272, 3) == 2 and W.wide_row_chunks(257, 273, 3) == 1
    assert [W.wide_row_chunks(n, 9) for n in (255, 256, 257, 513)] == [1, 1, 2, 3]
    assert [W.wide_row_chunks(n, 9, 3) for n in (255, 256, 257, 513)] == [1, 1, 2, 3]
    assert W.wide_width(512) == 256 and W.wide_width(513) == 1024


@pytest.mark.parametrize("mode", ["wnewton", "wmnewton"])
@pytest.mark.parametrize("name", W.LIST_CASES)
def test_list_cases_meet_their_conditions_and_stay_inside(mode, name):
    wn = mode == "wnewton"
    case, kw = (W.wn_list_case if wn else W.wmn_list_case)(name)
    kind = kw.pop("kind")
    pen = W.wn_pen(case.p) if wn else MN.penalised(case.K, case.p)
    for fsum in ORDERS:
        o, u = (_wn if wn else _wmn)(case, kind, fsum=fsum, **kw)
        s = o.solve
        if name == "second_screen_adds":
            assert s.converged and s.screens >= 2 and s.added[1] >= 1, s.added
            # ... among them coordinates of the high half of a 64-block, and the list is longer than one wavefront's ballot
            assert np.any(s.listed & (np.arange(len(pen)) % 64 >= 32)) and s.listed.sum() > 64
        elif name == "rests_at_zero":
            assert s.converged and np.any(s.listed & pen & (s.u == 0.0)), "no listed coordinate came to rest at an exact 0"
        elif name == "empty_list":
            assert kw["l2"] == 0.0 and not kw["ridge"] and not kw["fit_intercept"] and np.all(case.u_cur[pen] == 0.0)
            assert kw["l1"] > np.abs(o.q[pen]).max() and not s.listed.any()
            assert (s.sweeps, s.converged) == (1, True) and o.cd_u.tobytes() == case.u_cur.tobytes()
        elif name == "exhausted":
            assert not s.converged and s.sweeps == kw["max_sweeps"]
        elif name == "single_sweep":
            assert s.sweeps == 1
        elif name == "frozen_intercept":
            assert o.cd_u[~pen].tobytes() == case.u_cur[~pen].tobytes() and np.all(case.u_cur[~pen] != 0.0)
        held = dict(_held(kw), must_converge=name not in ("exhausted", "single_sweep"))
        (W.wn_check_probe if wn else W.wmn_check_probe)(o, case, u, 0.5, **held)


# (wrong version, the list case or count it is run on, the check that must fail); None: the scale pass alone is checked
WRONG = [("no_1_over_n", "second_screen_adds", "scale: H is not M / n"),
         ("s_j_squared", "second_screen_adds", "scale: H is not bitwise symmetric"),
         ("wrong_triangle", "second_screen_adds", "scale: H has a NaN"),
         ("q_from_ones", "second_screen_adds", "scale: q is not"),
         ("pad_nonzero", "second_screen_adds", "scale: the pad rows are not exactly 0.0"),
         ("no_rescreen", "second_screen_adds", "inner: coordinate .* misses optimality"),
         ("no_intercept_in_list", "second_screen_adds", "inner: coordinate .* misses optimality"),
         ("no_screen", "second_screen_adds", "inner: coordinate .* misses optimality"),
         ("high_word_lost", "second_screen_adds", "inner: coordinate .* misses optimality"),
         ("odd_last_not_moved", "odd_count", "inner: not converged")]          # (the intercept runs away: its g never moves)


def _wrong_case(mode, where):
    wn = mode == "wnewton"
    if where == "odd_count":                  # an odd count whose last coordinate, an intercept, is fitted
        case = W.wn_case(N_ROWS, 32, 1) if wn else W.wmn_case(N_ROWS, 10, 3, 1)
        assert (case.p + 1 if wn else case.Q) % 2 == 1
        l2, l1, ridge = W.MIX["mix0.5"]
        return case, "moderate", dict(l2=l2, l1=l1, ridge=ridge, fit_intercept=True, max_sweeps=1000, tol=1e-7)
    case, kw = (W.wn_list_case if wn else W.wmn_list_case)(where)
    return case, kw.pop("kind"), kw


WRONG_RUNS = [(m,) + w for m in ("wnewton", "wmnewton") for w in WRONG] + \
             [("wmnewton", "pair_not_reordered", "second_screen_adds", "scale: H is not")]       # (wnewton has no class pairs)


@pytest.mark.parametrize("mode,wrong,where,fails", WRONG_RUNS)
def test_wrong_versions_fall_outside(mode, wrong, where, fails):
    wn = mode == "wnewton"
    case, kind, kw = _wrong_case(mode, where)
    check = W.wn_check_probe if wn else W.wmn_check_probe
    o, u = (_wn if wn else _wmn)(case, kind, wrong=wrong, **kw)
    with pytest.raises(AssertionError, match=fails):
        check(o, case, u, 0.5, must_converge=True, **_held(kw))
    o, u = (_wn if wn else _wmn)(case, kind, **kw)
    check(o, case, u, 0.5, must_converge=True, **_held(kw))        # the right version on the same input stays inside


@pytest.mark.parametrize("mode", ["wnewton", "wmnewton"])
def test_single_sweep_is_the_list_sweep_not_the_full_one(mode):
    """a full narrow sweep moves coordinates the first screen left out: it falls outside the list-restricted reference"""
    wn = mode == "wnewton"
    case, kw = (W.wn_list_case if wn else W.wmn_list_case)("single_sweep")
    kind = kw.pop("kind")
    o, u = (_wn if wn else _wmn)(case, kind, **kw)
    (W.wn_check_probe if wn else W.wmn_check_probe)(o, case, u, 0.5, **_held(kw))
    a = (kw["l2"], kw["l1"], kw["ridge"], True, 1, kw["tol"])
    full = N.sweeps_f64(o.M, case.scale, case.n, case.u_cur, *a)[0] if wn else MN.sweeps_f64(o.M, case.scale, case.n, case.K, case.u_cur, *a)[0]
    assert not np.array_equal(full, o.cd_u)
    o.cd_u = full
    with pytest.raises(AssertionError, match="inner: single sweep"):
        W.check_list_solve(o, mode, W.wn_pen(case.p) if wn else MN.penalised(case.K, case.p), case.u_cur, kw["l2"], kw["l1"], kw["ridge"],
                           True, 1, kw["tol"])


def test_degenerate_inputs_follow_each_mode_s_rule():
    """a constant column without l2: to 0 in wnewton, stays in wmnewton; every weight 0: H = 0 and the intercept stays"""
    l2, l1, ridge = W.MIX["mix1"]
    case = W.wn_case(N_ROWS, 16, 1)
    a = W.constant_column(case)
    assert case.u_cur[a] != 0.0
    o, u = _wn(case, "moderate", "mix1")
    W.wn_check_probe(o, case, u, 0.5, l2, l1, ridge, must_converge=True)
    assert o.Hd[a] == 0.0 and o.q[a] == 0.0 and o.cd_u[a] == 0.0
    c = W.wmn_case(N_ROWS, 15, 3, 1)
    j = np.arange(c.K) * c.P + W.constant_column(c)
    assert np.all(c.u_cur[j] != 0.0)
    o, u = _wmn(c, "moderate", "mix1")
    W.wmn_check_probe(o, c, u, 0.5, l2, l1, ridge, must_converge=True)
    assert np.all(o.Hd[j] == 0.0) and o.cd_u[j].tobytes() == c.u_cur[j].tobytes()
    case = W.wn_case(N_ROWS, 16, 1)
    u = np.concatenate([np.zeros(case.p), [-800.0]])
    o = W.wn_restate(case, u, 0.5, l2, l1, ridge)
    W.wn_check_probe(o, case, u, 0.5, l2, l1, ridge)
    assert not o.H.any() and o.cd_u[case.p] == case.u_cur[case.p] and np.all(o.cd_u[:case.p] == 0.0)
    c = W.wmn_case(N_ROWS, 15, 3, 1)
    u = np.zeros(c.Q)
    u[c.p] = 800.0
    o = W.wmn_restate(c, u, 0.5, l2, l1, ridge)
    W.wmn_check_probe(o, c, u, 0.5, l2, l1, ridge)
    b = np.arange(c.Q) % c.P == c.p
    assert not o.H.any() and o.cd_u[b].tobytes() == c.u_cur[b].tobytes()


def test_wide_scale_gives_the_narrow_prologue_s_bits():
    """where both modes run: the wide H is, bit for bit, what the narrow kernels' prologue arithmetic gives on the same M"""
    case = W.wn_case(N_ROWS, 64, 1)
    o, _u = _wn(case, "moderate", "mix0.5", upto="scale")
    H, q = W.narrow_prologue_wn(o.M, case.scale, case.n)
    Hn, qn = N.model_from_M(o.M, case.scale, case.n)
    assert np.array_equal(o.H[:, :case.p + 1], H) and np.array_equal(o.q, q)
    assert np.all(np.abs(H.astype(N.LD) - Hn) <= 3 * N.U * np.abs(Hn)) and np.all(np.abs(q.astype(N.LD) - qn) <= 2 * N.U * np.abs(qn))
    c = W.wmn_case(N_ROWS, 21, 3, 1)
    o, _u = _wmn(c, "moderate", "mix0.5", upto="scale")
    H, q = W.narrow_prologue_wmn(o.M, c.scale, c.n, c.K)
    assert np.array_equal(o.H[:, :c.Q], H) and np.array_equal(o.q, q)


def test_sampled_moments_hold_what_the_full_check_holds():
    """the sampled check of the limit shapes on a small input: inside for the restatement, outside for a perturbed entry"""
    case = W.wn_case(N_ROWS, 40, 1)
    o, u = _wn(case, "moderate", "mix0.5", upto="scale")
    W.check_wn_moments_sampled(o, case)
    a, b = W.sample_positions(case.p + 2, case.p + 1, 1)
    o.M[a[0], b[0]] *= 1 + 1e-12
    with pytest.raises(AssertionError, match="moments: M"):
        W.check_wn_moments_sampled(o, case)
    c = W.wmn_case(N_ROWS, 20, 3, 1)
    o, u = _wmn(c, "moderate", "mix0.5", upto="scale")
    W.check_wmn_moments_sampled(o, c)
    a, b = W.sample_positions(c.p + 2, c.p + 1, 1 + 4)
    o.M[4, a[0], b[0]] *= 1 + 1e-12
    with pytest.raises(AssertionError, match="moments: M"):
        W.check_wmn_moments_sampled(o, c)


def test_probe_refusals_and_no_device():
    """the wide probes refuse by name what the plan refuses, before they look for a device; without one they say so"""
    import ctypes as C

    import sgdnet_amd as sa
    from sgdnet_amd import _lib, diagnostics
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sgdnet_hip.h")).read()
    assert "int sgdnet_wnewton_probe(" in hdr and "int sgdnet_wmnewton_probe(" in hdr and _lib.ABI_VERSION == 6
    L = sa.load()
    assert L.sgdnet_wnewton_max_features() == W.WNEWTON_MAX_FEATURES
    assert L.sgdnet_wmnewton_max_features(2) == W.WMNEWTON_MAX_COORDINATES // 2 - 1
    big = W.wn_case(3, W.WNEWTON_MAX_FEATURES + 1, 1)
    with pytest.raises(sa.SgdnetError, match=r"mode = wnewton needs no more features than sgdnet_wnewton_max_features\(\)") as e:
        diagnostics.wnewton_probe(big.x, big.y, big.scale, big.u_cur, big.u_cur)
    assert e.value.code == -5
    for K in (2, 3, 99, 100):
        limit = L.sgdnet_wmnewton_max_features(K)
        big = W.wmn_case(3, limit + 1, K, 1)
        with pytest.raises(sa.SgdnetError, match=r"mode = wmnewton needs no more features than sgdnet_wmnewton_max_features\(n_classes\)") as e:
            diagnostics.wmnewton_probe(big.x, big.y, K, big.scale, big.u_cur, big.u_cur)
        assert e.value.code == -5 and "(limit %d)" % limit in str(e.value)
    case, c = W.wn_case(20, 3, 1), W.wmn_case(20, 3, 3, 1)
    for kw in (dict(max_sweeps=0), dict(width=64), dict(width=512), dict(width=-256), dict(width=1)):
        with pytest.raises(sa.SgdnetError, match="sgdnet_wnewton_probe: invalid argument") as e:
            diagnostics.wnewton_probe(case.x, case.y, case.scale, case.u_cur, case.u_cur, **kw)
        assert e.value.code == -1
        with pytest.raises(sa.SgdnetError, match="sgdnet_wmnewton_probe: invalid argument") as e:
            diagnostics.wmnewton_probe(c.x, c.y, 3, c.scale, c.u_cur, c.u_cur, **kw)
        assert e.value.code == -1
    for K in (1, 0, -3):
        with pytest.raises(sa.SgdnetError, match="sgdnet_wmnewton_probe: invalid argument") as e:
            diagnostics.wmnewton_probe(c.x, c.y, K, c.scale, c.u_cur[:max(K, 0) * 4], c.u_cur[:max(K, 0) * 4])
        assert e.value.code == -1
    xf = np.asfortranarray(case.x)
    for fn, pr in ((L.sgdnet_wnewton_probe, _lib.WNewtonProbe()), (L.sgdnet_wmnewton_probe, _lib.WMNewtonProbe())):
        pr.max_sweeps = 10                                   # every pointer NULL
        if hasattr(pr, "K"):
            pr.K = 3
        assert fn(_lib.dptr(xf), 20, 3, 0, C.byref(pr)) == -1 and b"invalid argument" in L.sgdnet_last_error()
        assert fn(_lib.dptr(xf), 20, 3, 0, None) == -1 and b"invalid argument" in L.sgdnet_last_error()
        for n, p in ((0, 3), (20, 0)):
            assert fn(_lib.dptr(xf), n, p, 0, C.byref(pr)) == -1 and b"invalid matrix" in L.sgdnet_last_error()
        assert fn(None, 20, 3, 0, C.byref(pr)) == -1 and b"invalid matrix" in L.sgdnet_last_error()
    if L.sgdnet_device_count() == 0:
        with pytest.raises(sa.SgdnetError, match="no HIP device") as e:
            diagnostics.wnewton_probe(case.x, case.y, case.scale, case.u_cur, case.u_cur)
        assert e.value.code == -2
        with pytest.raises(sa.SgdnetError, match="no HIP device") as e:
            diagnostics.wmnewton_probe(c.x, c.y, 3, c.scale, c.u_cur, c.u_cur)
        assert e.value.code == -2
