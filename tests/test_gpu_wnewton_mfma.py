"""The matrix-core moments kernel of wide Newton mode (sgdnet_amd/csrc/newton_mfma.hip), selected by the option
"wnewton_moments" = 1: the pass through sgdnet_wnewton_probe against the exact references of tests/wide_passes_reference.py at
the kernel's own edges (tests/test_wnewton_mfma_reference.py has the shapes and proves the bounds on them on the CPU), a second
call bit for bit, the option's values, and sa.sgdnet_wnewton end to end against the optimality conditions and against the fit
with the option off."""
import numpy as np
import pytest

import newton_reference as N
import test_gpu_newton as tn
import test_gpu_wnewton as gw
import test_gpu_wnewton_passes as gp
import test_wnewton_mfma_reference as R
import wide_passes_reference as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import torch  # noqa: F401  -- before libsgdnet_hip.so (sgdnet_amd/_lib.py)
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    return sgdnet_amd


def _probe(sa, case, u):
    from sgdnet_amd import diagnostics
    with sa.option("wnewton_moments", 1):
        return diagnostics.wnewton_probe(case.x, case.y, case.scale, case.u_cur, u, t=0.5, centre=case.centre, max_sweeps=1, **R.PEN)


@pytest.mark.parametrize("n,p,centre", R.CASES)
def test_the_pass_against_the_exact_reference(sa, n, p, centre):
    """mean, v, r, loss, V, R and every defined entry of M inside the a-priori bounds of a sum in any order; the scale pass
    bit for bit on the M returned; one list sweep"""
    case = W.wn_case(n, p, centre)
    u = N.candidate(case, "moderate")
    W.wn_check_probe(_probe(sa, case, u), case, u, 0.5, max_sweeps=1, **R.PEN)


def test_the_feature_limit(sa):
    """p = 5819 at n = 40: 91 macro tiles, 4186 pairs in one chunk, the last macro tile 61 columns wide; checked as
    tests/test_gpu_wnewton_passes.py checks the tile kernel there (the moments on W.sample_positions)"""
    from sgdnet_amd import diagnostics
    case = W.wn_limit_case()
    u = N.candidate(case, "moderate")
    with sa.option("wnewton_moments", 1):
        o = diagnostics.wnewton_probe(case.x, case.y, case.scale, case.u_cur, u, t=0.5, centre=case.centre, **W.LIMIT_PENALTY)
    W.wn_check_probe(o, case, u, 0.5, sampled=True, must_converge=True, **W.LIMIT_PENALTY)


def test_a_second_call_returns_the_same_bits_and_the_option_is_checked(sa):
    case = W.wn_case(2 * R.C + 1, 2 * R.T - 1, 1)           # three chunks of three macro-tile pairs
    u = N.candidate(case, "moderate")
    gp._same_bits(_probe(sa, case, u), _probe(sa, case, u), case.p)
    assert sa.get_option("wnewton_moments") == 0
    for value in (2, -1):
        with pytest.raises(sa.SgdnetError):
            sa.set_option("wnewton_moments", value)
    assert sa.get_option("wnewton_moments") == 0


@pytest.mark.parametrize("shape,sparse", [((300, 70), False), ((65, 256), True)])
def test_the_fit_is_optimal_and_is_the_fit_of_the_tile_kernel(sa, shape, sparse):
    x, y = tn.problem(shape[0], shape[1], sparse)
    kw = dict(alpha=0.5, nlambda=10)
    with sa.option("wnewton_moments", 1):
        fit = gw.fit_and_check(sa, x, y, (shape, sparse, "wnewton_moments = 1"), **kw)
    off = sa.sgdnet_wnewton(x, y, **kw, **gw.KW)
    scale = np.abs(off.beta).max()
    print(shape, sparse, "matrix-core vs tile kernel: max coefficient difference / max|beta| = %.3g, npasses %g against %g"
          % (max(np.abs(fit.beta - off.beta).max(), np.abs(fit.a0 - off.a0).max()) / scale, fit.npasses, off.npasses))
    assert fit.lambda_.tobytes() == off.lambda_.tobytes()
    assert np.abs(fit.beta - off.beta).max() <= gw.SAME_OPTIMUM_REL * scale and np.abs(fit.a0 - off.a0).max() <= gw.SAME_OPTIMUM_REL * scale
