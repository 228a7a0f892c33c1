"""sa.kkt_from_gradient pins the driver's penalty conventions with no device involved: at the CPU oracle's optimum
(thresh = 1e-11, maxit = 5000, return_codes == 0) the certificate must be a convergence remainder, for every family,
with and without standardising, with and without an intercept, for ridge, elastic net, lasso and the group lasso.

The gradient comes from the numpy definition (tests/kkt_reference.py), so what is under test is the turning of
(G, G0) into a residual: sd(y), the feature means and sds, the group norms, the point at which a fit without an
intercept is stationary.

Cases: {gaussian, binomial, multinomial K = 3, mgaussian with 2 responses} x {standardize} x {intercept} x alpha in
{0, 0.5, 1}, on dense x (400 x 10), three lambdas below lambda_max each; and on sparse x wherever the reference
iteration has a fixed point to certify.  What the penalty or the iteration does not allow, found while writing this:
  * group lasso with a ridge part (mgaussian, alpha = 0.5): the reference's GroupLasso functor (src/penalties.h:61-79)
    compares the norm of the STORED coefficients with the threshold and shrinks by factor / w_scale; with a ridge part
    w_scale != 1 and the iteration has no fixed point (the oracle returns return_codes 1 after 5000 epochs, ratio ~ 1).
  * sparse x, standardize = True, alpha < 1: the oracle stops at 5000 epochs with return_codes 1 and ratio 2e-4
    (implicit centring next to the lazily applied ridge scaling); alpha = 1 converges and is kept.
  * lambda_max itself: the coefficients are 0 from the first epoch, the stopping rule looks at coefficients only, and
    the intercept is left where the first epochs' steps put it (residual up to 3e-3, and with it ratio 4e-5 for
    binomial): the lambdas here start at lambda_max / 2.

Observed on the CPU, largest `ratio` (= residual / lambda) and largest intercept residual over a family's cases:
    gaussian     ratio 1.5e-9    intercept 1.0e-8
    binomial     ratio 1.9e-10   intercept 4.4e-10
    multinomial  ratio 1.9e-10   intercept 1.6e-10
    mgaussian    ratio 3.7e-10   intercept 2.8e-9
The asserted bound is 10 x the family's figure (kkt_reference.RATIO_BOUND / INTERCEPT_BOUND; the remainder varies with
seed and conditioning), capped at 1e-5: an oracle that cannot stay under the cap means the convention is wrong, not
the cap.  A wrong convention (sd(y) left out, sds not applied, the group norm replaced by the entries) leaves ratios
of 1e-2 .. 1; the negative controls check that a 1 % change of one coefficient is seen (> 1e-3).
"""
import numpy as np
import pytest

import kkt_reference as KR

FAMILIES = ("gaussian", "binomial", "multinomial", "mgaussian")
SEEDS = {"gaussian": 11, "binomial": 12, "multinomial": 13, "mgaussian": 14}


def _cases():
    for family in FAMILIES:
        for sparse in (False, True):
            for standardize in (False, True):
                for intercept in (True, False):
                    for alpha in (0.0, 0.5, 1.0):
                        if family == "mgaussian" and alpha == 0.5:
                            continue                       # module docstring: no fixed point
                        if sparse and standardize and alpha < 1.0:
                            continue                       # module docstring: return_codes 1
                        yield pytest.param(family, sparse, standardize, intercept, alpha,
                                           id=f"{family}-{'sparse' if sparse else 'dense'}-std{int(standardize)}-"
                                              f"icpt{int(intercept)}-alpha{alpha}")


def _fit_and_certify(oracle, family, sparse, standardize, intercept, alpha, perturb=False):
    import sgdnet_amd as sa
    x, y = KR.problem(family, SEEDS[family], sparse=sparse)
    kw = dict(family=family, standardize=standardize, intercept=intercept, seed=3)
    lam_max = oracle.fit(x, y, alpha=1.0, nlambda=2, maxit=1, **kw)["lambda"][0]
    lam = lam_max * np.array([0.5, 0.15, 0.04]) / max(alpha, 0.25)
    res = oracle.fit(x, y, alpha=alpha, lambda_=lam, thresh=1e-11, maxit=5000, **kw)
    assert (res["return_codes"] == 0).all()
    fit = KR.as_fit(family, res, alpha)
    if perturb:
        beta = res["beta"].copy()
        k, j = np.argwhere(beta[:, :, -1] != 0)[0]
        beta[k, j, -1] *= 1.01
        fit.beta = beta
    x_center, x_scale = sa.feature_moments(x, standardize)
    y_center, y_scale = sa.response_moments(fit, y)
    a0 = sa.evaluation_intercepts(fit, x_center, y_center, intercept)
    G, G0, _, _ = KR.numpy_gradient(family, x, y, a0, np.asarray(fit.beta))
    return sa.kkt_from_gradient(G, G0, fit, x_center=x_center, x_scale=x_scale, y_scale=y_scale,
                                standardize=standardize, intercept=intercept), fit


@pytest.mark.parametrize("family,sparse,standardize,intercept,alpha", list(_cases()))
def test_certificate_at_the_oracle_optimum(oracle, family, sparse, standardize, intercept, alpha):
    out, fit = _fit_and_certify(oracle, family, sparse, standardize, intercept, alpha)
    print(f"kkt {family} sparse={sparse} std={standardize} icpt={intercept} alpha={alpha}: ratio {out['ratio'].max():.3e} "
          f"intercept {out['intercept'].max():.3e}")
    assert out["ratio"].shape == out["coef"].shape == out["intercept"].shape == fit.lambda_.shape
    assert np.array_equal(out["ratio"], out["coef"] / fit.lambda_)
    assert out["ratio"].max() < KR.RATIO_BOUND[family]
    assert out["intercept"].max() < KR.INTERCEPT_BOUND[family]
    if not intercept:
        assert (out["intercept"] == 0).all()
    assert np.count_nonzero(np.asarray(fit.beta)[:, :, -1]) > 0       # inside the active set: not a test of zeros only
    if alpha == 1.0:
        assert (np.asarray(fit.beta)[:, :, 0] == 0).any()             # ... and of exact zeros too


@pytest.mark.parametrize("family", FAMILIES)
def test_a_perturbed_coefficient_is_seen(oracle, family):
    out, _ = _fit_and_certify(oracle, family, False, True, True, 1.0, perturb=True)
    print(f"kkt {family} perturbed: ratio at the last lambda {out['ratio'][-1]:.3e}")
    assert out["ratio"][-1] > 1e-3
    assert out["ratio"][:-1].max() < KR.RATIO_BOUND[family]      # the other lambdas are untouched
