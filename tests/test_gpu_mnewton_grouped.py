"""sa.sgdnet_mnewton / sa.sgdnet_wmnewton with type_multinomial="grouped" (sgdnet_amd/csrc/mnewton_grouped.hip) against the
plain numpy reference of tests/mnewton_grouped_reference.py.  The bounds are 4 x the worst value measured on an MI355X over
the cases of this file (profiles/mnewton_grouped.txt):
    KKT residual / lambda      worst 2.47e-10  (the ungrouped modes' own on the same shapes and thresh: 5.67e-9)
    objective - reference's    worst 4.44e-16
    coefficients, alpha = 1    worst 5.99e-11 of the path's max|w|; |sum_k w_kj| worst 7.43e-15 of it
    wide against narrow        worst 2.33e-15 of max|beta|
Both widths of either inner solve (the options "mnewton_width", "wmnewton_width") give the same bits."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import mnewton_grouped_reference as gr

pytestmark = pytest.mark.gpu
KKT_BOUND, OBJECTIVE_BOUND, COEF_BOUND, CENTRE_BOUND, WIDE_BOUND = 4 * 2.47e-10, 4 * 4.44e-16, 4 * 5.99e-11, 4 * 7.43e-15, 4 * 2.33e-15
UNGROUPED = "needs the ungrouped penalty (type_multinomial = 0)"
CASES = [("mnewton", s) for s in gr.SHAPES] + [("wmnewton", s) for s in gr.SHAPES + gr.WIDE_ONLY]


@pytest.fixture(scope="module")
def sa():
    import torch  # noqa: F401
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    return sgdnet_amd


_solved = {}


def reference(shape, mix, intercept, lambdas):
    """the reference's [(W, b, residual)] on this path, solved once per (shape, mix, intercept, path)"""
    key = (shape, mix, intercept, lambdas.tobytes())
    if key not in _solved:
        x, y = gr.problem(*shape)
        _solved[key] = gr.solve(gr.standardised(x)[0], y, shape[2], lambdas, mix, intercept)
    return _solved[key]


def fit_grouped(sa, mode, shape, mix, intercept=True, x=None):
    """alpha = 1: 8 user lambdas from the grouped lambda_max down; else the driver's automatic path of 8"""
    xd, y = gr.problem(*shape)
    kw = dict(alpha=mix, intercept=intercept, thresh=gr.THRESH, type_multinomial="grouped")
    if mix == 1.0:
        kw["lambda_"] = gr.user_lambdas(gr.standardised(xd)[0], y, shape[2], mix, intercept)
    else:
        kw.update(nlambda=gr.N_LAMBDA, lambda_min_ratio=gr.MIN_RATIO)
    fit = getattr(sa, "sgdnet_" + mode)(xd if x is None else x, y, **kw)
    assert (fit.return_codes == 0).all() and fit.grouped and fit.draws_used == 0
    return fit


def same_bits(a, b):
    return all(np.asarray(getattr(a, f)).tobytes() == np.asarray(getattr(b, f)).tobytes() for f in ("beta", "a0", "dev_ratio", "lambda_", "npasses"))


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("mix", gr.MIXES)
@pytest.mark.parametrize("mode,shape", CASES)
def test_grouped_fit_is_the_grouped_optimum(sa, mode, shape, mix, intercept):
    x, y = gr.problem(*shape)
    z, m, s = gr.standardised(x)
    fit = fit_grouped(sa, mode, shape, mix, intercept)
    ref = reference(shape, mix, intercept, fit.lambda_)
    B = np.stack(fit.beta)                                               # (K, p, L)
    size = max(np.abs(Wr).max() for Wr, _, _ in ref)                    # of the path: at lambda_max the reference holds rounding
    kkt = obj = coef = centre = 0.0
    for l, ((Wr, br, res), lam) in enumerate(zip(ref, fit.lambda_)):
        W, b = (B[:, :, l] * s).T, np.asarray(fit.a0)[:, l] + (B[:, :, l] @ m if intercept else 0.0)      # the reference's coordinates
        assert res <= gr.FLOOR
        assert ((W == 0).all(1) | (W != 0).all(1)).all()                 # (d) a feature's classes are zero together
        kkt = max(kkt, gr.kkt_residual(z, y, W, b, lam, mix, intercept) / lam)
        obj = max(obj, gr.objective(z, y, W, b, lam, mix) - gr.objective(z, y, Wr, br, lam, mix))
        coef = max(coef, np.abs(W - Wr).max() / size)
        centre = max(centre, np.abs(W.sum(1)).max() / size)
    device = sa.kkt(fit, x, y, intercept=intercept, grouped=True)["ratio"].max()
    print("FIGURES", mode, shape, mix, intercept, "kkt/lambda %.3g (sa.kkt %.3g) objective %.3g coef %.3g centre %.3g npasses %g"
          % (kkt, device, obj, coef, centre, fit.npasses))
    assert kkt <= KKT_BOUND and device <= KKT_BOUND                      # (a)
    assert obj <= OBJECTIVE_BOUND                                        # (b)
    if mix == 1.0:                                                       # (c); and the path starts at lambda_max: at exact zeros
        assert coef <= COEF_BOUND and centre <= CENTRE_BOUND and (B[:, :, 0] == 0).all()


@pytest.mark.parametrize("mix", gr.MIXES)
@pytest.mark.parametrize("shape", gr.SHAPES)
def test_wide_and_narrow_reach_the_same_optimum(sa, shape, mix):
    narrow, wide = fit_grouped(sa, "mnewton", shape, mix), fit_grouped(sa, "wmnewton", shape, mix)
    assert narrow.lambda_.tobytes() == wide.lambda_.tobytes()
    diff = np.abs(np.stack(wide.beta) - np.stack(narrow.beta)).max() / np.abs(np.stack(narrow.beta)).max()
    print("FIGURES wide vs narrow", shape, mix, "%.3g of max|beta|" % diff)
    assert diff <= WIDE_BOUND


@pytest.mark.parametrize("mode,widths,shape", [("mnewton", (64, 256), (200, 33, 3)), ("mnewton", (64, 256), (300, 65, 3)),
                                               ("wmnewton", (256, 1024), (120, 5, 3)), ("wmnewton", (256, 1024), (300, 70, 3)),
                                               ("wmnewton", (256, 1024), (200, 40, 5))])
def test_both_widths_give_the_same_bits(sa, mode, widths, shape):
    fits = []
    for width in widths:
        with sa.option(mode + "_width", width):
            fits.append(fit_grouped(sa, mode, shape, 0.5))
    assert same_bits(*fits) and fits[0].npasses > 0


@pytest.mark.parametrize("mode,shape", [("mnewton", (200, 33, 3)), ("wmnewton", (300, 70, 3))])
def test_sparse_x_gives_the_dense_bits(sa, mode, shape):
    x, _ = gr.problem(*shape)
    x[np.abs(x) < 1.0] = 0.0
    assert same_bits(fit_grouped(sa, mode, shape, 0.5, x=sp.csc_matrix(x)), fit_grouped(sa, mode, shape, 0.5, x=x))


@pytest.mark.parametrize("mode", ["mnewton", "wmnewton"])
def test_alpha_zero_is_the_ungrouped_fit(sa, mode):
    x, y = gr.problem(120, 5, 3)
    kw = dict(alpha=0, nlambda=gr.N_LAMBDA, thresh=gr.THRESH)
    assert same_bits(getattr(sa, "sgdnet_" + mode)(x, y, type_multinomial="grouped", **kw), getattr(sa, "sgdnet_" + mode)(x, y, **kw))


def test_refusals_stay(sa):
    """the option at 0: type_multinomial = 1 through the native entry is refused as ever; the grouped cross-validation is
    refused with the option at 1"""
    from sgdnet_amd import _lib
    x, y = gr.problem(120, 5, 3)
    L, xf, buf = sa.load(), np.asfortranarray(x), np.zeros(256)

    def control(**fields):
        ctl = _lib.Control()
        ctl.family, ctl.intercept, ctl.standardize, ctl.max_iter, ctl.tol, ctl.n_lambda, ctl.n_classes, ctl.type_multinomial = 2, 1, 1, 100, 1e-7, 2, 3, 1
        for k, v in fields.items():
            setattr(ctl, k, v)
        return ctl

    assert sa.get_option("mnewton_grouped") == 0
    for mode in (_lib.MODE_MNEWTON, _lib.MODE_WMNEWTON):
        res = _lib.Result()
        res.a0, res.beta, res.lambda_, res.dev_ratio, res.return_codes = [_lib.dptr(buf)] * 5
        rc = L.sgdnet_fit_dense(_lib.dptr(xf), 120, 5, _lib.dptr(y), 1, C.byref(control(elasticnet_mix=0.5, lambda_min_ratio=0.1, mode=mode)), C.byref(res))
        assert rc == -5 and UNGROUPED in L.sgdnet_last_error().decode()
    with sa.option("mnewton_grouped", 1):
        fold, alphas, lam = np.ascontiguousarray(np.arange(120) % 3, dtype=np.int32), np.array([0.5]), np.array([[0.1, 0.01]])
        rc = L.sgdnet_cv_mnewton_dense(_lib.dptr(xf), 120, 5, _lib.dptr(y), fold.ctypes.data_as(C.POINTER(C.c_int32)), 3, 0, C.byref(control()), 1,
                                       _lib.dptr(alphas), _lib.dptr(lam), C.byref(_lib.CvMNewtonResult(*[_lib.dptr(buf)] * 8)))
        assert rc == -5 and UNGROUPED in L.sgdnet_last_error().decode()
