"""The passes of one outer step of multinomial Newton mode (sgdnet_amd/csrc/mnewton.hip) one by one, through
sgdnet_mnewton_probe, against exact references (tests/mnewton_reference.py).

The end-to-end tests (tests/test_gpu_mnewton.py) cannot see the curvature side: the fixed point of a proximal Newton
iteration depends on the gradient terms alone, and a wrong weight, a wrong entry or class block of H, or a wrong scaling
of H only costs steps, sweeps or halvings.  Here every pass is held to the long-double truth formed from what the pass
before it RETURNED, inside rounding-error bounds composed over the kernel's own arithmetic (the derivations are in
mnewton_reference's docstring; none was taken from what a device returned, and tests/test_mnewton_reference.py shows on
the CPU that float64 restatements in three summation orders stay inside them on these very inputs while ten wrong
formulas do not):

  bitwise   the published candidate and its a = u / scale, the blend at t = 1 and at t = 0.5, change and size, mu = 0
            where exp underflows, the q column of every off-diagonal class pair, the frozen intercepts, a coordinate
            without curvature, the two widths of the inner solve against each other, every output on a second call
  bounded   mean, mu (absolute bounds where a class underflows; each row sums to 1), the loss (finite at |eta| = 800),
            every defined entry of every class pair's M, the penalty sums of the record, the optimality of the inner
            solve for the joint model of the returned M wherever the solve is known to converge (the flag is asserted
            first), a single sweep against long double and numpy elsewhere"""
import numpy as np
import pytest

import mnewton_reference as R

pytestmark = pytest.mark.gpu

MIX = dict((name, (l2, l1, ridge)) for name, l2, l1, ridge in R.PENALTIES)
EDGE_RUNS = R.runs(R.EDGE_SHAPES)
LIMIT_RUNS = R.runs(R.LIMIT_SHAPES, kinds=("moderate", "wide", "overflow"), centres=(1,))


@pytest.fixture(scope="module")
def probe():
    import torch  # noqa: F401  -- before libsgdnet_hip.so (sgdnet_amd/_lib.py)
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    for K, limit in R.MAX_FEATURES.items():
        assert sgdnet_amd.mnewton_max_features(K) == limit
    from sgdnet_amd import diagnostics
    return diagnostics


def _run(probe, case, u, pen, t=0.5, **kw):
    l2, l1, ridge = MIX[pen]
    o = probe.mnewton_probe(case.x, case.y, case.K, case.scale, case.u_cur, u, t=t, centre=case.centre, l2=l2, l1=l1, ridge=ridge, **kw)
    return o, (l2, l1, ridge)


def _probe_and_check(probe, case, kind, pen, t=0.5, **kw):
    """kw: fit_intercept, max_sweeps, width; a case that is known to converge is held to the flag, then to optimality"""
    u = R.candidate(case, kind)
    plan = dict(R.solve_plan(case, kind, pen))
    if "max_sweeps" in kw:
        plan = dict(max_sweeps=kw["max_sweeps"])
    width = kw.pop("width", 0)
    o, (l2, l1, ridge) = _run(probe, case, u, pen, t, width=width, **dict(kw, max_sweeps=plan["max_sweeps"]))
    R.check_probe(o, case, u, t, l2, l1, ridge, **dict(kw, **plan))
    return o


@pytest.mark.parametrize("n,p,K,centre,kind,pen", EDGE_RUNS)
def test_tile_and_row_edges(probe, n, p, K, centre, kind, pen):
    """p + 2 on both sides of a 16-column tile; n on both sides of the 64-row step, one, two and three chunks, several
    workgroups of the state pass at 1025; the penalties rotate with the candidates and the shapes"""
    o = _probe_and_check(probe, R.case(n, p, K, centre), kind, pen)
    if kind == "overflow":
        assert np.isfinite(o.loss) and np.all(np.isfinite(o.mu))


@pytest.mark.parametrize("n,p,K,centre,kind,pen", LIMIT_RUNS)
def test_class_count_and_lds_edges(probe, n, p, K, centre, kind, pen):
    """the feature limit at K = 2, 3, 10 (Q = 198, 198, 190) and K = 99 (Q = 198, 4950 class pairs in gridDim.z)"""
    case = R.case(n, p, K, centre)
    o = _probe_and_check(probe, case, kind, pen)
    assert o.M.shape == (K * (K + 1) // 2, case.p + 2, case.p + 2)


@pytest.mark.parametrize("pen", list(MIX))
@pytest.mark.parametrize("n,p,K", R.STRIDE_SHAPES)
def test_inner_solve_across_the_lane_stride(probe, n, p, K, pen):
    """Q = 63, 64, 65: the 64-lane striding of the load, of the g update and of mnewton_publish, and the width rule; with
    and without the intercepts (frozen: bitwise unchanged); one sweep only"""
    case = R.case(n, p, K, 1)
    assert case.Q == (63, 64, 65)[R.STRIDE_SHAPES.index((n, p, K))]
    for kw in (dict(), dict(fit_intercept=False), dict(max_sweeps=1)):
        o = _probe_and_check(probe, case, "moderate", pen, **kw)
        if kw.get("fit_intercept") is False:
            b = np.arange(case.Q) % case.P == case.p
            assert o.cd_u[b].tobytes() == case.u_cur[b].tobytes()
        if "max_sweeps" in kw:
            assert o.cd_rec["sweeps"] == 1.0


@pytest.mark.parametrize("n,p,K", [(80, 20, 3), (80, 12, 5), (300, None, 2), (130, 1, 99)])
def test_both_widths_give_the_same_bits(probe, n, p, K):
    """Q = 63, 65, 198 and K = 99: one wavefront and 256 lanes leave byte-identical candidates and records"""
    case = R.case(n, p, K, 1)
    a = _probe_and_check(probe, case, "moderate", "mix0.5", width=64)
    b = _probe_and_check(probe, case, "moderate", "mix0.5", width=256)
    _same_bits(a, b)


def test_a_class_without_a_member(probe):
    case = R.case(65, 15, 3, 1, empty_class=1)
    assert not np.any(case.y == 1)
    _probe_and_check(probe, case, "moderate", "mix0.5")


@pytest.mark.parametrize("pen", ["mix1", "mix0.5"])
def test_constant_column(probe, pen):
    """its H and q entries are 0.0 in every pair; without an l2 term its coordinate stays at u_cur in every class, bitwise;
    with one it becomes 0.0"""
    case = R.case(65, 15, 3, 1)
    case.xd[:, 2] = 3.0
    j = np.arange(case.K) * case.P + 2
    assert np.all(case.u_cur[j] != 0.0)
    o = _probe_and_check(probe, case, "moderate", pen)
    assert np.all(o.M[:, :3, 2] == 0.0) and np.all(o.M[:, 2, 2:] == 0.0)
    if MIX[pen][0] == 0.0:
        assert o.cd_u[j].tobytes() == case.u_cur[j].tobytes()
    else:
        assert np.all(o.cd_u[j] == 0.0)


@pytest.mark.parametrize("pen", ["mix0.5", "mix1"])
def test_one_class_at_800_on_every_row(probe, pen):
    """mu is exactly 1 and 0, every H entry is 0.0, the loss is finite, the intercepts have no curvature and stay"""
    case = R.case(65, 15, 3, 1)
    u = np.zeros(case.Q)
    u[case.p] = 800.0
    o, (l2, l1, ridge) = _run(probe, case, u, pen)
    R.check_probe(o, case, u, 0.5, l2, l1, ridge)
    assert np.all(o.mu[:, 0] == 1.0) and np.all(o.mu[:, 1:] == 0.0) and np.isfinite(o.loss)
    H = o.M[:, :case.P, :case.P]
    assert np.all(H[:, np.triu(np.ones((case.P, case.P), dtype=bool))] == 0.0)
    b = np.arange(case.Q) % case.P == case.p
    assert o.cd_u[b].tobytes() == case.u_cur[b].tobytes()


@pytest.mark.parametrize("t", [1.0, 0.5, 0.3])
def test_blend(probe, t):
    """t = 1: the candidate comes back bitwise; 0.5: exact scaling, bitwise; 0.3: three roundings"""
    case = R.case(65, 15, 3, 1)
    o = _probe_and_check(probe, case, "moderate", "mix0.5", t=t)
    if t == 1.0:
        assert np.array_equal(o.blend_u, o.pub_u) and np.array_equal(o.blend_a, o.pub_a) and o.blend_rec == o.pub_rec


def _same_bits(a, b):
    K, p = a.mu.shape[1], a.mean.shape[0]
    k = R.defined(K, p)
    for name in ("mean", "pub_u", "pub_a", "blend_u", "blend_a", "mu", "cd_u", "cd_a"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert a.M[k].tobytes() == b.M[k].tobytes(), "M"
    assert np.float64(a.loss).tobytes() == np.float64(b.loss).tobytes(), "loss"
    for name in ("pub_rec", "blend_rec", "cd_rec"):
        assert getattr(a, name) == getattr(b, name), name


def test_a_second_call_returns_the_same_bits(probe):
    case = R.case(1025, 33, 3, 1)
    u = R.candidate(case, "wide")
    a, _ = _run(probe, case, u, "mix0.5")
    b, _ = _run(probe, case, u, "mix0.5")
    _same_bits(a, b)


def test_probe_refuses_what_the_plan_refuses(probe):
    import sgdnet_amd as sa
    for K in (2, 10, 99, 100):
        case = R.case(20, sa.mnewton_max_features(K) + 1, K, 1)
        with pytest.raises(sa.SgdnetError, match=r"mode = mnewton needs no more features than sgdnet_mnewton_max_features\(n_classes\)") as e:
            _run(probe, case, R.candidate(case, "zero"), "mix0.5")
        assert e.value.code == -5
    case = R.case(20, 3, 3, 1)
    for kw in (dict(max_sweeps=0), dict(width=128)):
        with pytest.raises(sa.SgdnetError, match="sgdnet_mnewton_probe: invalid argument") as e:
            _run(probe, case, R.candidate(case, "zero"), "mix0.5", **kw)
        assert e.value.code == -1
    with pytest.raises(sa.SgdnetError, match="sgdnet_mnewton_probe: invalid argument") as e:
        probe.mnewton_probe(case.x, case.y, 1, case.scale, case.u_cur[:4], case.u_cur[:4])
    assert e.value.code == -1
