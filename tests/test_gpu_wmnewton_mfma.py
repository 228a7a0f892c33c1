"""The matrix-core class-pair moments kernel of wide multinomial Newton mode (sgdnet_amd/csrc/mnewton_mfma.hip), selected by the
option "wmnewton_moments" = 1: the pass through sgdnet_wmnewton_probe against the exact references of
tests/wide_passes_reference.py and tests/mnewton_reference.py at the kernel's own edges (their moment bounds hold for a sum in any
order), a second call bit for bit, the option's values, and sa.sgdnet_wmnewton end to end against the optimality conditions and
against the fit with the option off."""
import numpy as np
import pytest

import mnewton_reference as MN
import test_gpu_wmnewton as gw
import test_gpu_wmnewton_passes as gp
import wide_passes_reference as W
import wmnewton_reference as wr

pytestmark = pytest.mark.gpu

T, S, C, G = 64, 32, 256, 6     # csrc/wide_layout.hpp: kMfmaTileCols, kMfmaSlabRows, kMfmaMinChunkRows; csrc/mnewton.hpp: kWmnewtonMfmaGroup
# (n, p, K): p + 2 on either side of a 16-column tile and of a macro tile -- "ones" and "r" in one macro tile (64: p = 62, p + 1
# = 63) and apart (65: p = 63 | p + 1 = 64), a diagonal macro pair alone (<= 64) and with off-diagonal ones (129: three tiles)
COLUMNS = [(48, nc - 2, 3) for nc in (3, 16, 17, T - 1, T, T + 1, T + 2, 2 * T + 1)]
# the instruction's depth (4) and the slab; one, two and three chunks, the last holding one row
ROWS = [(n, 7, 2) for n in (1, 3, 4, 5, S - 1, S, S + 1, C, C + 1, 2 * C + 1)]
# 3, 6, 10 and 15 class pairs: less than a group, exactly one, and one and two groups with a partial last one
CLASSES = [(48, 7, K) for K in (2, 3, 4, 5)]
CASES = [(n, p, K, i % 2) for i, (n, p, K) in enumerate(COLUMNS + ROWS + CLASSES + [(48, W.WMN_MANY_CLASSES[1], W.WMN_MANY_CLASSES[0])])]


@pytest.fixture(scope="module")
def sa():
    import torch  # noqa: F401  -- before libsgdnet_hip.so (sgdnet_amd/_lib.py)
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    return sgdnet_amd


def _probe(sa, c, u, **kw):
    from sgdnet_amd import diagnostics
    with sa.option("wmnewton_moments", 1):
        return diagnostics.wmnewton_probe(c.x, c.y, c.K, c.scale, c.u_cur, u, t=0.5, centre=c.centre, **kw)


@pytest.mark.parametrize("n,p,K,centre", CASES)
def test_the_pass_against_the_exact_reference(sa, n, p, K, centre):
    """mean, mu, loss and every defined entry of every pair's M inside the a-priori bounds of a sum in any order; the scale
    pass bit for bit on the M returned; one list sweep"""
    pairs = [k * (k + 1) // 2 for _, _, k in CLASSES]
    assert min(pairs) < G and G in pairs and any(G < c < 2 * G for c in pairs) and any(c > 2 * G and c % G for c in pairs)
    c = W.wmn_case(n, p, K, centre)
    u = MN.candidate(c, "moderate")
    l2, l1, ridge = W.MIX["mix0.5"]
    W.wmn_check_probe(_probe(sa, c, u, l2=l2, l1=l1, ridge=ridge, max_sweeps=1), c, u, 0.5, l2, l1, ridge, max_sweeps=1)


def test_the_coordinate_limit(sa):
    """K = 2, p = 2909 at n = 40: 46 macro tiles, 1081 pairs in one chunk, a group of three class pairs; checked as
    tests/test_gpu_wmnewton_passes.py checks the tile kernel there (the moments on W.sample_positions)"""
    c = W.wmn_limit_case()
    u = MN.candidate(c, "moderate")
    W.wmn_check_probe(_probe(sa, c, u, **W.WMN_LIMIT_PENALTY), c, u, 0.5, sampled=True, must_converge=True, **W.WMN_LIMIT_PENALTY)


def test_a_second_call_returns_the_same_bits_and_the_option_is_checked(sa):
    c = W.wmn_case(2 * C + 1, 2 * T - 1, 3, 1)              # three chunks of six macro-tile pairs, one full group
    u = MN.candidate(c, "moderate")
    gp._same_bits(_probe(sa, c, u, l2=0.025, l1=0.025), _probe(sa, c, u, l2=0.025, l1=0.025))
    assert sa.get_option("wmnewton_moments") == 0
    for value in (2, -1):
        with pytest.raises(sa.SgdnetError):
            sa.set_option("wmnewton_moments", value)
    assert sa.get_option("wmnewton_moments") == 0


@pytest.mark.parametrize("shape,sparse", [((300, 70), False), ((65, 256), True)])
def test_the_fit_is_optimal_and_is_the_fit_of_the_tile_kernel(sa, shape, sparse):
    x, y = wr.problem(shape[0], shape[1], 3, sparse=sparse)
    kw = dict(alpha=0.5, nlambda=10)
    with sa.option("wmnewton_moments", 1):
        fit = gw.fit_and_check(sa, x, y, (shape, sparse, "wmnewton_moments = 1"), **kw)
    off = sa.sgdnet_wmnewton(x, y, **kw, **gw.KW)
    scale = np.abs(gw.stacked(off)).max()
    coef = np.abs(gw.stacked(fit) - gw.stacked(off)).max() / scale
    icpt = np.abs(np.asarray(fit.a0) - np.asarray(off.a0)).max() / scale
    ddev = np.abs(fit.dev_ratio - off.dev_ratio).max()
    print(shape, sparse, "matrix-core vs tile kernel: coefficients %.3g intercepts %.3g of max|beta|, dev_ratio %.3g, npasses %g against %g"
          % (coef, icpt, ddev, fit.npasses, off.npasses))
    assert fit.lambda_.tobytes() == off.lambda_.tobytes()
    assert coef <= gw.SAME_OPTIMUM_REL and icpt <= gw.SAME_OPTIMUM_REL
    assert ddev <= gw.SAME_DEV_RATIO
