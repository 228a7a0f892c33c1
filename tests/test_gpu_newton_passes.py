"""The passes of one outer step of Newton mode (sgdnet_amd/csrc/newton.hip) one by one, through sgdnet_newton_probe_dense /
_sparse, against exact references (tests/newton_reference.py).

The end-to-end tests (tests/test_gpu_newton.py) cannot see the curvature side: the fixed point of a proximal Newton
iteration depends on the gradient terms alone, and a wrong v, H, V or a wrong scaling of H only costs steps.  Here every
pass is held to the long-double truth formed from what the pass before it RETURNED, inside rounding-error bounds
composed over the kernel's own arithmetic (the derivations are in newton_reference's docstring; none was taken from
what a device returned, and tests/test_newton_reference.py shows on the CPU that float64 restatements in three summation
orders stay inside them on these very inputs while seven wrong formulas do not):

  bitwise   the published candidate and its a = u / scale, the blend at t = 1 and at t = 0.5, change and size, the
            corners of M, the frozen intercept, a coordinate without curvature, every output on a second call
  bounded   mean, v, r (absolute bounds), loss, V, R, every defined entry of M, the penalty sums of the record, the
            optimality of the inner solve for the model of the returned M, a single sweep against long double and numpy"""
import numpy as np
import pytest

import newton_reference as R

pytestmark = pytest.mark.gpu

MIX = dict((name, (l2, l1, ridge)) for name, l2, l1, ridge in R.PENALTIES)
PENS = list(MIX)
KINDS = list(R.CANDIDATES)


@pytest.fixture(scope="module")
def probe():
    import torch  # noqa: F401  -- before libsgdnet_hip.so (sgdnet_amd/_lib.py)
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    assert sgdnet_amd.newton_max_features() == R.MAX_FEATURES
    from sgdnet_amd import diagnostics
    return diagnostics


def _run(probe, case, u, pen, t=0.5, **kw):
    l2, l1, ridge = MIX[pen]
    o = probe.newton_probe(case.x, case.y, case.scale, case.u_cur, u, t=t, centre=case.centre, l2=l2, l1=l1, ridge=ridge, **kw)
    return o, (l2, l1, ridge)


def _probe_and_check(probe, case, kind, pen, t=0.5, **kw):
    u = R.candidate(case, kind)
    o, (l2, l1, ridge) = _run(probe, case, u, pen, t, **kw)
    R.check_probe(o, case, u, t, l2, l1, ridge, **kw)
    return o


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("centre", [0, 1])
@pytest.mark.parametrize("n,p", R.DENSE_SHAPES)
def test_dense_passes(probe, n, p, centre, kind):
    """p + 1 and p + 2 on both sides of a 16-column tile, n on both sides of the 64-row step and of one chunk / two
    chunks, the feature limit; the penalties rotate with the candidates"""
    o = _probe_and_check(probe, R.dense_case(n, p, centre), kind, PENS[KINDS.index(kind) % 3])
    if kind == "overflow" and n > 1:
        assert o.loss == np.inf or np.all(np.isfinite(o.v))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("centre", [0, 1])
@pytest.mark.parametrize("n", R.SPARSE_N)
def test_sparse_passes(probe, n, centre, kind):
    """columns that are empty, full, one entry, longer than a workgroup, of identical and of disjoint supports, with
    stored zeros, and of mean 1e6"""
    _probe_and_check(probe, R.sparse_case(n, centre), kind, PENS[(KINDS.index(kind) + 1) % 3])


@pytest.mark.parametrize("centre", [0, 1])
@pytest.mark.parametrize("n", [257, 600])
def test_descending_rows_give_the_bits_of_ascending_rows(probe, n, centre):
    """the AscendingColumns copy: the same matrix with every column's rows stored in descending order"""
    up, down = R.sparse_case(n, centre), R.sparse_case(n, centre, descending=True)
    assert np.array_equal(up.xd, down.xd) and not np.array_equal(up.x.indices, down.x.indices)
    u = R.candidate(up, "moderate")
    a, _ = _run(probe, up, u, "mix0.5")
    b = _probe_and_check(probe, down, "moderate", "mix0.5")
    _same_bits(a, b, up.p)


@pytest.mark.parametrize("centre", [0, 1])
def test_sparse_matrix_that_stores_nothing(probe, centre):
    for kind in ("zero", "moderate"):
        o = _probe_and_check(probe, R.empty_sparse_case(255, 3, centre), kind, "mix0.5")
        assert np.all(o.mean == 0.0) and np.all(o.M[:3, :3][np.triu_indices(3)] == 0.0)


@pytest.mark.parametrize("pen", PENS)
@pytest.mark.parametrize("n,p", [(80, 1), (80, 63), (80, 64), (80, 65), (300, None)])
def test_inner_solve_across_the_lane_stride(probe, n, p, pen):
    """p = 1, 63, 64, 65 and the limit: the 64-lane striding of the load, of the g update and of publish_candidate; with
    and without the intercept (frozen: bitwise unchanged); one sweep only"""
    case = R.dense_case(n, p, 1)
    for kw in (dict(), dict(fit_intercept=False), dict(max_sweeps=1)):
        o = _probe_and_check(probe, case, "moderate", pen, **kw)
        if kw.get("fit_intercept") is False:
            assert o.cd_u[case.p] == case.u_cur[case.p]
        if "max_sweeps" in kw:
            assert o.cd_rec["sweeps"] == 1.0


def test_constant_column_without_l2_goes_to_zero(probe):
    case = R.dense_case(65, 16, 1)
    case.xd[:, 2] = 3.0
    case.x = case.xd
    assert case.u_cur[2] != 0.0
    o = _probe_and_check(probe, case, "moderate", "mix1")
    assert o.M[2, 2] == 0.0 and o.M[2, case.p + 1] == 0.0 and o.cd_u[2] == 0.0


@pytest.mark.parametrize("pen", ["mix0.5", "mix1"])
def test_all_weights_zero_leaves_the_intercept(probe, pen):
    """eta = -800 on every row: t = 1, v = 0 exactly, H = 0; the intercept has no curvature and stays"""
    case = R.dense_case(65, 16, 1)
    u = np.concatenate([np.zeros(case.p), [-800.0]])
    o, (l2, l1, ridge) = _run(probe, case, u, pen)
    R.check_probe(o, case, u, 0.5, l2, l1, ridge)
    assert np.all(o.v == 0.0) and o.V == 0.0 and np.isfinite(o.loss)
    assert np.all(o.M[:case.p + 1, :case.p + 1][np.triu_indices(case.p + 1)] == 0.0)
    assert o.cd_u[case.p] == case.u_cur[case.p]
    if l2 == 0.0:
        assert np.all(o.cd_u[:case.p] == 0.0)


@pytest.mark.parametrize("t", [1.0, 0.5, 0.3])
def test_blend(probe, t):
    """t = 1: the candidate comes back bitwise; 0.5: exact scaling, bitwise; 0.3: three roundings"""
    case = R.dense_case(65, 16, 1)
    o = _probe_and_check(probe, case, "moderate", "mix0.5", t=t)
    if t == 1.0:
        assert np.array_equal(o.blend_u, o.pub_u) and np.array_equal(o.blend_a, o.pub_a) and o.blend_rec == o.pub_rec


def _same_bits(a, b, p):
    k = R.upper(p + 2)
    for name in ("mean", "pub_u", "pub_a", "blend_u", "blend_a", "v", "r", "cd_u", "cd_a"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert a.M[k].tobytes() == b.M[k].tobytes(), "M"
    for name in ("loss", "V", "R"):
        assert np.float64(getattr(a, name)).tobytes() == np.float64(getattr(b, name)).tobytes(), name
    for name in ("pub_rec", "blend_rec", "cd_rec"):
        assert getattr(a, name) == getattr(b, name), name


@pytest.mark.parametrize("layout", ["dense", "sparse"])
def test_a_second_call_returns_the_same_bits(probe, layout):
    case = R.dense_case(1025, 33, 1) if layout == "dense" else R.sparse_case(600, 1)
    u = R.candidate(case, "wide")
    a, _ = _run(probe, case, u, "mix0.5")
    b, _ = _run(probe, case, u, "mix0.5")
    _same_bits(a, b, case.p)


def test_probe_refuses_what_the_plan_refuses(probe):
    import sgdnet_amd as sa
    case = R.dense_case(20, R.MAX_FEATURES + 1, 1)
    with pytest.raises(sa.SgdnetError, match=r"mode = newton needs no more features than sgdnet_newton_max_features\(\)") as e:
        _run(probe, case, R.candidate(case, "zero"), "mix0.5")
    assert e.value.code == -5
    case = R.dense_case(20, 3, 1)
    with pytest.raises(sa.SgdnetError, match="invalid argument") as e:
        _run(probe, case, R.candidate(case, "zero"), "mix0.5", max_sweeps=0)
    assert e.value.code == -1
