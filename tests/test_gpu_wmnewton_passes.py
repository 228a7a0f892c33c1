"""The passes of one outer step of wide multinomial Newton mode (sgdnet_amd/csrc/mnewton.hip: wmnewton_run's steps) one by
one, through sgdnet_wmnewton_probe, against exact references (tests/wide_passes_reference.py, tests/mnewton_reference.py).

What tests/test_gpu_wnewton_passes.py says of the binomial mode holds here over the Q = K (p + 1) joint coordinates: the
path tests (tests/test_gpu_wmnewton.py) cannot see a joint H that is not symmetric, has a class pair on the wrong side of
the diagonal or a dirty pad, a coordinate the list lost or a re-screen that never runs, and beyond 199 / K - 1 features no
narrow fit exists to compare with.  Every pass is held to a reference formed from what the pass before it RETURNED; no
tolerance was taken from a device run (tests/test_wide_passes_reference.py is the CPU proof on these very inputs).

  bitwise   the scale pass in full (every class block of H in the kernel's order of operations, symmetric, the pad rows
            exactly 0.0, ld, diag H, q); the published candidate and its a, the blend at t = 1 and 0.5, change and size; mu
            = 0 where exp underflows; the q column of the off-diagonal pairs; frozen intercepts; a coordinate without
            curvature; the three widths against each other in every output; a second call; the wide H against the narrow
            prologue's arithmetic on the same M
  bounded   mean, mu, loss and every defined entry of every pair's M as MN.check_probe holds them; the optimality of the
            list solve over ALL coordinates for the returned H and q; one list sweep against long double and numpy
Each check prints the value closest to its bound (run with -s)."""
import numpy as np
import pytest

import mnewton_reference as MN
import wide_passes_reference as W

pytestmark = pytest.mark.gpu

N_ROWS = 48          # tests/test_wide_passes_reference.py proves the bounds on these very cases
COUNT_RUNS = W.count_runs(W.WMN_SHAPES + [W.WMN_MANY_CLASSES])


@pytest.fixture(scope="module")
def probe():
    import torch  # noqa: F401  -- before libsgdnet_hip.so (sgdnet_amd/_lib.py)
    import sgdnet_amd
    L = sgdnet_amd.load()
    if L.sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    assert L.sgdnet_wmnewton_max_features(2) == W.WMNEWTON_MAX_COORDINATES // 2 - 1
    assert L.sgdnet_wmnewton_max_features(3) == W.WMNEWTON_MAX_COORDINATES // 3 - 1
    from sgdnet_amd import diagnostics
    return diagnostics


def _run(probe, c, u, t=0.5, **kw):
    return probe.wmnewton_probe(c.x, c.y, c.K, c.scale, c.u_cur, u, t=t, centre=c.centre, **kw)


def _held(kw):
    return {k: v for k, v in kw.items() if k in ("l2", "l1", "ridge", "fit_intercept", "max_sweeps", "tol")}


def _probe_and_check(probe, c, kind, pen, t=0.5, sampled=False, **kw):
    """a case the plan holds to convergence is held to the flag, then to optimality; the others to one list sweep"""
    l2, l1, ridge = W.MIX[pen]
    plan = W.solve_plan(kind, pen, c.n, c.Q)
    if "max_sweeps" in kw:
        plan = dict(max_sweeps=kw.pop("max_sweeps"))
    u = MN.candidate(c, kind)
    o = _run(probe, c, u, t, l2=l2, l1=l1, ridge=ridge, max_sweeps=plan["max_sweeps"], **kw)
    W.wmn_check_probe(o, c, u, t, l2, l1, ridge, sampled=sampled, **dict(_held(kw), **plan))
    return o


def _same_bits(a, b):
    K, p = a.mu.shape[1], a.mean.shape[0]
    k = MN.defined(K, p)
    for name in ("mean", "pub_u", "pub_a", "blend_u", "blend_a", "mu", "H", "Hd", "q", "cd_u", "cd_a"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert a.M[k].tobytes() == b.M[k].tobytes(), "M"
    assert np.float64(a.loss).tobytes() == np.float64(b.loss).tobytes(), "loss"
    for name in ("pub_rec", "blend_rec", "cd_rec"):
        assert getattr(a, name) == getattr(b, name), name
    assert a.ld == b.ld


@pytest.mark.parametrize("shape,centre,kind,pen", COUNT_RUNS)
def test_coordinate_counts(probe, shape, centre, kind, pen):
    """Q = K (p + 1) on either side of what wide_layout.hpp and wide_cd_device.hpp branch on (W.WMN_SHAPES says which
    counts exist and what stands in for the primes 17 and 257), with K = 2 and K = 3 wherever the count divides -- c % P puts
    an intercept at every block end, K = 3, p = 1: coordinates 1, 3, 5 -- and K = 20, p = 12: many classes, few features.
    Width 0 is checked in full, and the two forced widths return its bits in every output."""
    K, p = shape
    c = W.wmn_case(N_ROWS, p, K, centre)
    o = _probe_and_check(probe, c, kind, pen)
    l2, l1, ridge = W.MIX[pen]
    ms = W.solve_plan(kind, pen, c.n, c.Q)["max_sweeps"]
    u = MN.candidate(c, kind)
    for width in (256, 1024):
        _same_bits(o, _run(probe, c, u, l2=l2, l1=l1, ridge=ridge, max_sweeps=ms, width=width))


@pytest.mark.parametrize("ncols", [272, 273])
def test_row_chunks_on_either_side_of_1024_workgroups(probe, ncols):
    """K = 2 (3 class pairs), n = 257: at p + 2 = 272 there are 17 tiles, 153 tile pairs, 459 workgroups a chunk and two row
    chunks; at 273, 18 tiles, 171 pairs, 513 workgroups and ONE chunk (mnewton.hpp: wmnewton_row_chunks: 1024 / 513 = 1).
    The moments are held on W.sample_positions for every class pair; the scale pass is checked in full."""
    assert W.wide_row_chunks(257, ncols, 3) == (2 if ncols == 272 else 1)
    _probe_and_check(probe, W.wmn_case(257, ncols - 2, 2, 1), "moderate", "mix0.5", sampled=True, max_sweeps=1)


@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_row_chunks_at_a_small_p(probe, n):
    """one chunk up to 256 rows, two at 257 (the second holds one row), three at 513; every entry of every pair's M"""
    assert W.wide_row_chunks(n, 9, 3) == {255: 1, 256: 1, 257: 2, 513: 3}[n]
    _probe_and_check(probe, W.wmn_case(n, 7, 2, n % 2), "wide", "mix0.5")


def test_the_coordinate_limit(probe):
    """K = 2, p = 2909, Q = 5820 at n = 40: ld = 5824 with 4 pad rows, 1024 lanes, the LDS budget of the list solve to its last
    bytes.  To stay within seconds: the scale outputs are checked bitwise IN FULL in float64 and the list solve's optimality
    over all 5820 coordinates; the moments only on W.sample_positions of every class pair (the corners, the last tile's
    edges and 4000 seeded entries, not all 25 million in long double)."""
    c = W.wmn_limit_case()
    assert c.n == 40 and c.Q == W.WMNEWTON_MAX_COORDINATES and W.leading_dim(c.Q) == 5824
    u = MN.candidate(c, "moderate")
    o = _run(probe, c, u, **W.WMN_LIMIT_PENALTY)
    W.wmn_check_probe(o, c, u, 0.5, sampled=True, must_converge=True, **W.WMN_LIMIT_PENALTY)


@pytest.mark.parametrize("name", W.LIST_CASES)
def test_list_cases(probe, name):
    """the second screen adds coordinates; a listed coordinate rests at an exact 0; the empty list (one sweep, converged, u
    unchanged); max_sweeps exhausted; one list sweep against the list-restricted reference; the frozen intercepts.  That
    the inputs meet these conditions is asserted on the CPU (tests/test_wide_passes_reference.py)."""
    c, kw = W.wmn_list_case(name)
    u = MN.candidate(c, kw.pop("kind"))
    o = _run(probe, c, u, **kw)
    W.wmn_check_probe(o, c, u, 0.5, must_converge=name not in ("exhausted", "single_sweep"), **_held(kw))
    rec = o.cd_rec
    pen = MN.penalised(c.K, c.p)
    if name == "empty_list":
        assert (rec["sweeps"], rec["converged"]) == (1.0, 1.0) and o.cd_u.tobytes() == c.u_cur.tobytes()
    elif name == "exhausted":
        assert (rec["sweeps"], rec["converged"]) == (3.0, 0.0)
    elif name == "single_sweep":
        assert rec["sweeps"] == 1.0
    elif name == "frozen_intercept":
        assert o.cd_u[~pen].tobytes() == c.u_cur[~pen].tobytes()
    elif name == "rests_at_zero":
        assert np.any(pen & (c.u_cur != 0.0) & (o.cd_u == 0.0))
    for width in (256, 1024):
        _same_bits(o, _run(probe, c, u, width=width, **kw))


@pytest.mark.parametrize("pen", ["mix1", "mix0.5"])
def test_constant_column(probe, pen):
    """mnewton_coord_new_u's rule: without an l2 term the coordinate stays at u_cur in every class, bitwise
    (newton_coord_new_u sends it to 0); with one it becomes 0.0.  Its row and column of H are 0.0 in every class block"""
    c = W.wmn_case(N_ROWS, 15, 3, 1)
    j = np.arange(c.K) * c.P + W.constant_column(c)
    o = _probe_and_check(probe, c, "moderate", pen)
    assert not o.H[j].any() and not o.H[:, j].any() and not o.q[j].any()
    if W.MIX[pen][0] == 0.0:
        assert o.cd_u[j].tobytes() == c.u_cur[j].tobytes()
    else:
        assert np.all(o.cd_u[j] == 0.0)


@pytest.mark.parametrize("pen", ["mix0.5", "mix1"])
def test_one_class_at_800_on_every_row(probe, pen):
    """mu is exactly 1 and 0, every weight is 0: H = 0 in every entry; the intercepts have no curvature and stay"""
    c = W.wmn_case(N_ROWS, 15, 3, 1)
    l2, l1, ridge = W.MIX[pen]
    u = np.zeros(c.Q)
    u[c.p] = 800.0
    o = _run(probe, c, u, l2=l2, l1=l1, ridge=ridge)
    W.wmn_check_probe(o, c, u, 0.5, l2, l1, ridge)
    assert np.all(o.mu[:, 0] == 1.0) and np.all(o.mu[:, 1:] == 0.0) and np.isfinite(o.loss)
    assert not o.H.any() and not o.Hd.any()
    b = ~MN.penalised(c.K, c.p)
    assert o.cd_u[b].tobytes() == c.u_cur[b].tobytes()


@pytest.mark.parametrize("t", [1.0, 0.5, 0.3])
def test_blend(probe, t):
    """mnewton_wide_blend_kernel forms the blend where it is read.  t = 1: the candidate comes back bitwise; 0.5: exact
    scaling, bitwise; 0.3: three roundings.  Q = 99: the second stride of the publishing wavefront"""
    c = W.wmn_case(N_ROWS, 32, 3, 1)
    o = _probe_and_check(probe, c, "moderate", "mix0.5", t=t)
    if t == 1.0:
        assert np.array_equal(o.blend_u, o.pub_u) and np.array_equal(o.blend_a, o.pub_a) and o.blend_rec == o.pub_rec


@pytest.mark.parametrize("K,p", [(3, 21), (3, 65)])
def test_narrow_against_wide(probe, K, p):
    """where both modes run (Q = 66, and 198 at K = 3's narrow limit; at K = 2's the list solve needs more than the 1000 sweeps): each M inside its own moment bounds, so the two within
    the sum of both (not bitwise: the row chunks differ); the wide H is bitwise what mnewton_cd_solve's prologue arithmetic
    gives on the wide M"""
    c = W.wmn_case(300, p, K, 1)
    u = MN.candidate(c, "moderate")
    l2, l1, ridge = W.MIX["mix0.5"]
    w = _run(probe, c, u, l2=l2, l1=l1, ridge=ridge)
    nar = probe.mnewton_probe(c.x, c.y, K, c.scale, c.u_cur, u, centre=c.centre, l2=l2, l1=l1, ridge=ridge)
    assert w.mu.tobytes() == nar.mu.tobytes() and w.mean.tobytes() == nar.mean.tobytes()
    ref = MN.check_moments(w, c)
    k = MN.defined(K, p)
    MN.inside(nar.M, ref, "moments: the narrow M", k)
    assert np.all(np.abs(w.M.astype(MN.LD) - nar.M.astype(MN.LD))[k] <= 2 * ref.e[k])
    H, q = W.narrow_prologue_wmn(w.M, c.scale, c.n, K)
    assert np.array_equal(w.H[:, :c.Q], H) and np.array_equal(w.q, q)
    W.wmn_check_probe(w, c, u, 0.5, l2, l1, ridge, must_converge=True)


def test_a_second_call_returns_the_same_bits(probe):
    c = W.wmn_case(513, 85, 3, 1)
    u = MN.candidate(c, "wide")
    a = _run(probe, c, u, l2=0.025, l1=0.025)
    b = _run(probe, c, u, l2=0.025, l1=0.025)
    _same_bits(a, b)


def test_probe_refuses_what_the_plan_refuses(probe):
    import sgdnet_amd as sa
    for K in (2, 3, 99, 100):
        c = W.wmn_case(3, sa.load().sgdnet_wmnewton_max_features(K) + 1, K, 1)
        with pytest.raises(sa.SgdnetError, match=r"mode = wmnewton needs no more features than sgdnet_wmnewton_max_features\(n_classes\)") as e:
            _run(probe, c, MN.candidate(c, "zero"))
        assert e.value.code == -5
    c = W.wmn_case(20, 3, 3, 1)
    for kw in (dict(max_sweeps=0), dict(width=64), dict(width=512)):
        with pytest.raises(sa.SgdnetError, match="sgdnet_wmnewton_probe: invalid argument") as e:
            _run(probe, c, MN.candidate(c, "zero"), **kw)
        assert e.value.code == -1
    with pytest.raises(sa.SgdnetError, match="sgdnet_wmnewton_probe: invalid argument") as e:
        probe.wmnewton_probe(c.x, c.y, 1, c.scale, c.u_cur[:4], c.u_cur[:4])
    assert e.value.code == -1
