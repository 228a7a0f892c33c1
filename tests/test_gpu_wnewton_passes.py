"""The passes of one outer step of wide Newton mode (sgdnet_amd/csrc/newton.hip: wnewton_run's steps) one by one, through
sgdnet_wnewton_probe, against exact references (tests/wide_passes_reference.py, tests/newton_reference.py).

The end-to-end tests (tests/test_gpu_wnewton.py) cannot see the curvature side: the fixed point of a proximal Newton
iteration depends on the gradient terms alone, and an H that is not symmetric, is scaled wrongly or has a dirty pad, a
coordinate the list lost or a re-screen that never runs only costs steps -- and beyond 198 features there is no narrow fit to
compare with.  Here every pass is held to a reference formed from what the pass before it RETURNED; no tolerance was taken
from a device run, and tests/test_wide_passes_reference.py shows on the CPU that float64 restatements in three summation
orders pass these very checks on these very inputs while eleven wrong versions do not.

  bitwise   the scale pass in full (H = M / n / (s s') in the kernel's order of operations, symmetric, the pad rows exactly
            0.0, ld, diag H, q); the published candidate and its a = u / scale, the blend at t = 1 and t = 0.5, change and
            size; a frozen intercept; the three widths (0, 256, 1024) against each other in every output; a second call;
            the wide H against the narrow prologue's arithmetic on the same M
  bounded   mean, v, r, loss, V, R and every defined entry of M as N.check_probe holds them (the wide mode's row chunks
            are another any-order sum); the optimality of the list solve over ALL coordinates for the returned H and q
            (the check that sees a coordinate the list lost), one list sweep against long double and numpy
Each check prints the value closest to its bound (run with -s)."""
import numpy as np
import pytest

import newton_reference as N
import wide_passes_reference as W

pytestmark = pytest.mark.gpu

N_ROWS = 48          # tests/test_wide_passes_reference.py proves the bounds on these very cases
COUNT_RUNS = W.count_runs(W.WN_COUNTS)


@pytest.fixture(scope="module")
def probe():
    import torch  # noqa: F401  -- before libsgdnet_hip.so (sgdnet_amd/_lib.py)
    import sgdnet_amd
    L = sgdnet_amd.load()
    if L.sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    assert L.sgdnet_wnewton_max_features() == W.WNEWTON_MAX_FEATURES and L.sgdnet_newton_max_features() == N.MAX_FEATURES
    from sgdnet_amd import diagnostics
    return diagnostics


def _run(probe, case, u, t=0.5, **kw):
    return probe.wnewton_probe(case.x, case.y, case.scale, case.u_cur, u, t=t, centre=case.centre, **kw)


def _held(kw):
    return {k: v for k, v in kw.items() if k in ("l2", "l1", "ridge", "fit_intercept", "max_sweeps", "tol")}


def _probe_and_check(probe, case, kind, pen, t=0.5, sampled=False, **kw):
    """a case the plan holds to convergence is held to the flag, then to optimality; the others to one list sweep"""
    l2, l1, ridge = W.MIX[pen]
    plan = W.solve_plan(kind, pen, case.n, case.p + 1)
    if "max_sweeps" in kw:
        plan = dict(max_sweeps=kw.pop("max_sweeps"))
    u = N.candidate(case, kind)
    o = _run(probe, case, u, t, l2=l2, l1=l1, ridge=ridge, max_sweeps=plan["max_sweeps"], **kw)
    W.wn_check_probe(o, case, u, t, l2, l1, ridge, sampled=sampled, **dict(_held(kw), **plan))
    return o


def _same_bits(a, b, p):
    k = N.upper(p + 2)
    for name in ("mean", "pub_u", "pub_a", "blend_u", "blend_a", "v", "r", "H", "Hd", "q", "cd_u", "cd_a"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert a.M[k].tobytes() == b.M[k].tobytes(), "M"
    for name in ("loss", "V", "R"):
        assert np.float64(getattr(a, name)).tobytes() == np.float64(getattr(b, name)).tobytes(), name
    for name in ("pub_rec", "blend_rec", "cd_rec"):
        assert getattr(a, name) == getattr(b, name), name
    assert a.ld == b.ld


@pytest.mark.parametrize("P,centre,kind,pen", COUNT_RUNS)
def test_coordinate_counts(probe, P, centre, kind, pen):
    """P = p + 1 on either side of what wide_layout.hpp and wide_cd_device.hpp branch on (W.WN_COUNTS says what each count
    sits on: the pad, the words of `bits`, the wavefronts' ballots, the compaction steps of either width), odd and even
    for wide_column_move's last slot; width 0 is checked in full, and the two forced widths return its bits in every
    output.  Candidates, penalties and centring rotate with the counts."""
    case = W.wn_case(N_ROWS, P - 1, centre)
    assert W.leading_dim(P) - P == (0 if P % 16 == 0 else 16 - P % 16)
    o = _probe_and_check(probe, case, kind, pen)
    l2, l1, ridge = W.MIX[pen]
    ms = W.solve_plan(kind, pen, case.n, P)["max_sweeps"]
    u = N.candidate(case, kind)
    for width in (256, 1024):
        _same_bits(o, _run(probe, case, u, l2=l2, l1=l1, ridge=ridge, max_sweeps=ms, width=width), case.p)


@pytest.mark.parametrize("ncols", [496, 497])
def test_row_chunks_on_either_side_of_1024_workgroups(probe, ncols):
    """n = 257 at p + 2 = 496: 31 tiles, 496 tile pairs, two row chunks (the second holds one row); at 497: 32 tiles, 528
    pairs, ONE chunk (wide_layout.hpp: wide_row_chunks).  The moments are held on W.sample_positions (the corners, the last
    tile's edges, 4000 seeded entries): every entry goes through the same chunking, and all 123 000 in long double take
    too long for a test; the scale pass is checked in full."""
    assert W.wide_row_chunks(257, ncols) == (2 if ncols == 496 else 1)
    _probe_and_check(probe, W.wn_case(257, ncols - 2, 1), "moderate", "mix0.5", sampled=True, max_sweeps=1)


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_row_chunks_at_a_small_p(probe, n):
    """one chunk up to 256 rows, two at 257 (the second holds one row), three at 513; every entry of M"""
    assert W.wide_row_chunks(n, 9) == {255: 1, 256: 1, 257: 2, 513: 3}[n]
    _probe_and_check(probe, W.wn_case(n, 7, n % 2), "wide", "mix0.5")


def test_the_feature_limit(probe):
    """p = 5819 at n = 40: 364 tiles, 66 430 tile pairs in one chunk, ld = 5824 with 4 pad rows, 1024 lanes, the LDS budget of
    the list solve to its last bytes.  To stay within seconds: the scale outputs are checked bitwise IN FULL in float64 and
    the list solve's optimality over all 5820 coordinates; the moments only on W.sample_positions (the corners, the last
    tile's edges and 4000 seeded entries, not all 34 million in long double)."""
    case = W.wn_limit_case()
    assert case.n == 40 and W.leading_dim(case.p + 1) == 5824 and W.wide_row_chunks(40, case.p + 2) == 1
    u = N.candidate(case, "moderate")
    o = _run(probe, case, u, **W.LIMIT_PENALTY)
    W.wn_check_probe(o, case, u, 0.5, sampled=True, must_converge=True, **W.LIMIT_PENALTY)


@pytest.mark.parametrize("name", W.LIST_CASES)
def test_list_cases(probe, name):
    """the second screen adds coordinates; a listed coordinate rests at an exact 0; the empty list (one sweep, converged, u
    unchanged); max_sweeps exhausted; one list sweep against the list-restricted reference; the frozen intercept.  That the
    inputs meet these conditions is asserted on the CPU (tests/test_wide_passes_reference.py)."""
    case, kw = W.wn_list_case(name)
    u = N.candidate(case, kw.pop("kind"))
    o = _run(probe, case, u, **kw)
    W.wn_check_probe(o, case, u, 0.5, must_converge=name not in ("exhausted", "single_sweep"), **_held(kw))
    rec = o.cd_rec
    if name == "empty_list":
        assert (rec["sweeps"], rec["converged"]) == (1.0, 1.0) and o.cd_u.tobytes() == case.u_cur.tobytes()
    elif name == "exhausted":
        assert (rec["sweeps"], rec["converged"]) == (3.0, 0.0)
    elif name == "single_sweep":
        assert rec["sweeps"] == 1.0
    elif name == "frozen_intercept":
        assert o.cd_u[case.p:].tobytes() == case.u_cur[case.p:].tobytes()
    elif name == "rests_at_zero":
        assert np.any((case.u_cur[:case.p] != 0.0) & (o.cd_u[:case.p] == 0.0))
    for width in (256, 1024):
        _same_bits(o, _run(probe, case, u, width=width, **kw), case.p)


def test_constant_column_without_l2_goes_to_zero(probe):
    """newton_coord_new_u's rule: no curvature, no l2 term: 0.0 (mnewton_coord_new_u lets it stay)"""
    case = W.wn_case(N_ROWS, 16, 1)
    a = W.constant_column(case)
    o = _probe_and_check(probe, case, "moderate", "mix1")
    assert o.M[a, a] == 0.0 and o.Hd[a] == 0.0 and not o.H[a].any() and o.q[a] == 0.0 and o.cd_u[a] == 0.0


@pytest.mark.parametrize("pen", ["mix0.5", "mix1"])
def test_all_weights_zero_leaves_the_intercept(probe, pen):
    """eta = -800 on every row: v = 0 exactly, H = 0 in every entry; the intercept has no curvature and stays"""
    case = W.wn_case(N_ROWS, 16, 1)
    l2, l1, ridge = W.MIX[pen]
    u = np.concatenate([np.zeros(case.p), [-800.0]])
    o = _run(probe, case, u, l2=l2, l1=l1, ridge=ridge)
    W.wn_check_probe(o, case, u, 0.5, l2, l1, ridge)
    assert np.all(o.v == 0.0) and not o.H.any() and not o.Hd.any()
    assert o.cd_u[case.p] == case.u_cur[case.p]
    if l2 == 0.0:
        assert np.all(o.cd_u[:case.p] == 0.0)


@pytest.mark.parametrize("t", [1.0, 0.5, 0.3])
def test_blend(probe, t):
    """newton_wide_blend_kernel forms the blend where it is read.  t = 1: the candidate comes back bitwise; 0.5: exact
    scaling, bitwise; 0.3: three roundings.  P = 100: the second stride of the publishing wavefront"""
    case = W.wn_case(N_ROWS, 99, 1)
    o = _probe_and_check(probe, case, "moderate", "mix0.5", t=t)
    if t == 1.0:
        assert np.array_equal(o.blend_u, o.pub_u) and np.array_equal(o.blend_a, o.pub_a) and o.blend_rec == o.pub_rec


@pytest.mark.parametrize("p", [64, 198])
def test_narrow_against_wide(probe, p):
    """where both modes run: each M inside its own moment bounds, so the two within the sum of both (not bitwise: the row
    chunks differ); the wide H is bitwise what newton_cd_solve's prologue arithmetic gives on the wide M"""
    case = W.wn_case(300, p, 1)
    u = N.candidate(case, "moderate")
    l2, l1, ridge = W.MIX["mix0.5"]
    w = _run(probe, case, u, l2=l2, l1=l1, ridge=ridge)
    nar = probe.newton_probe(case.x, case.y, case.scale, case.u_cur, u, centre=case.centre, l2=l2, l1=l1, ridge=ridge)
    assert w.v.tobytes() == nar.v.tobytes() and w.r.tobytes() == nar.r.tobytes() and w.mean.tobytes() == nar.mean.tobytes()
    ref = N.check_moments(w, case)
    k = N.upper(p + 2)
    N.inside(nar.M, ref, "moments: the narrow M", k)
    assert np.all(np.abs(w.M.astype(N.LD) - nar.M.astype(N.LD))[k] <= 2 * ref.e[k])
    H, q = W.narrow_prologue_wn(w.M, case.scale, case.n)
    assert np.array_equal(w.H[:, :p + 1], H) and np.array_equal(w.q, q)
    W.wn_check_probe(w, case, u, 0.5, l2, l1, ridge, must_converge=True)


def test_a_second_call_returns_the_same_bits(probe):
    case = W.wn_case(513, 257, 1)
    u = N.candidate(case, "wide")
    a = _run(probe, case, u, l2=0.025, l1=0.025)
    b = _run(probe, case, u, l2=0.025, l1=0.025)
    _same_bits(a, b, case.p)


def test_probe_refuses_what_the_plan_refuses(probe):
    import sgdnet_amd as sa
    case = W.wn_case(3, W.WNEWTON_MAX_FEATURES + 1, 1)
    with pytest.raises(sa.SgdnetError, match=r"mode = wnewton needs no more features than sgdnet_wnewton_max_features\(\)") as e:
        _run(probe, case, N.candidate(case, "zero"))
    assert e.value.code == -5
    case = W.wn_case(20, 3, 1)
    for kw in (dict(max_sweeps=0), dict(width=64), dict(width=512)):
        with pytest.raises(sa.SgdnetError, match="sgdnet_wnewton_probe: invalid argument") as e:
            _run(probe, case, N.candidate(case, "zero"), **kw)
        assert e.value.code == -1
