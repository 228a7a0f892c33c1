"""sa.sgdnet_wcovariance (SGDNET_MODE_WCOVARIANCE, sgdnet_amd/csrc/covariance.hip: wide_scale_kernel and
cov_wide_path_kernel): the gaussian path of one response solved to its optimum with the scaled Gram matrix in global
memory, for up to wcovariance_max_features() features.  Checked against the optimality conditions of the problem the
driver solves (sa.kkt), as tests/test_gpu_covariance.py checks mode = "covariance", and against that mode where both run.
The shapes sit at the kernels' edges (wcovariance_reference.SHAPES); tests/test_wcovariance_host.py runs the numpy
restatement of the algorithm on the same inputs on the CPU."""
import numpy as np
import pytest
import scipy.sparse as sp

import test_gpu_covariance as tc
import wcovariance_reference as wr

pytestmark = pytest.mark.gpu
KW = dict(thresh=wr.THRESH, maxit=wr.MAXIT)


@pytest.fixture(scope="module")
def sa():
    import torch  # noqa: F401
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    return sgdnet_amd


def same_bits(a, b):
    return (a.beta.tobytes() == b.beta.tobytes() and a.a0.tobytes() == b.a0.tobytes() and a.dev_ratio.tobytes() == b.dev_ratio.tobytes()
            and a.lambda_.tobytes() == b.lambda_.tobytes() and a.npasses == b.npasses and (a.return_codes == b.return_codes).all())


def fit_and_check(sa, x, y, what, standardize=True, intercept=True, **kw):
    fit = sa.sgdnet_wcovariance(x, y, standardize=standardize, intercept=intercept, **KW, **kw)
    assert (fit.return_codes == 0).all() and fit.draws_used == 0 and np.isfinite(fit.dev_ratio).all(), (what, fit.return_codes)
    tc.assert_optimal(sa.kkt(fit, x, y, standardize=standardize, intercept=intercept), fit.lambda_, what)
    return fit


# ---- (i) optimality across the envelope ----

def test_limit_is_the_one_the_host_test_derives(sa):
    assert sa.wcovariance_max_features() == wr.LIMIT >= 4096


@pytest.mark.parametrize("mix", wr.MIXES)
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", wr.SHAPES)
def test_automatic_path_is_optimal(sa, shape, sparse, mix):
    n, p = shape[0], shape[1] or sa.wcovariance_max_features()
    x, y = tc.problem(n, p, sparse)
    nlambda, ratio = wr.path_of(shape[0], shape[1], mix)
    for intercept, standardize in wr.settings_of(shape[1]):
        fit_and_check(sa, x, y, (n, p, sparse, mix, intercept, standardize), standardize, intercept, alpha=mix, nlambda=nlambda,
                      lambda_min_ratio=ratio)


@pytest.mark.parametrize("sparse", [False, True])
def test_large_mean_column_does_not_cancel(sa, sparse):
    x, y = wr.large_mean_problem(sparse)
    fit_and_check(sa, x, y, ("mean 1e6", sparse), alpha=0.5, nlambda=6, lambda_min_ratio=1e-2)


# ---- (ii) the same answer as mode = "covariance" where both run ----

@pytest.mark.parametrize("mix", [0.5, 0.0])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", [(600, 198), (200, 33)])
def test_same_optimum_as_covariance_mode(sa, shape, sparse, mix):
    x, y = tc.problem(shape[0], shape[1], sparse, seed=3)
    kw = dict(alpha=mix, nlambda=6, lambda_min_ratio=1e-2, **KW)
    wide, cov = sa.sgdnet_wcovariance(x, y, **kw), sa.sgdnet(x, y, mode="covariance", **kw)
    assert (wide.return_codes == 0).all() and (cov.return_codes == 0).all()
    assert wide.lambda_.tobytes() == cov.lambda_.tobytes() and wide.nulldev == cov.nulldev
    scale = np.abs(cov.beta).max()
    print(shape, sparse, mix, "wide vs covariance: max coefficient difference / max|beta| = %.3g, dev_ratio %.3g"
          % (max(np.abs(wide.beta - cov.beta).max(), np.abs(wide.a0 - cov.a0).max()) / scale, np.abs(wide.dev_ratio - cov.dev_ratio).max()))
    assert np.abs(wide.beta - cov.beta).max() <= 1e-9 * scale and np.abs(wide.a0 - cov.a0).max() <= 1e-9 * scale
    assert np.abs(wide.dev_ratio - cov.dev_ratio).max() <= 1e-10


# ---- (iii) determinism: the workgroup's width, and a second call ----

# (40, limit): the instance that requests the next column while a move updates the gradient (beyond 1536 features)
@pytest.mark.parametrize("shape, sparse", [((65, 1025), False), ((65, 1025), True), ((63, 15), False), ((63, 15), True), ((40, None), False)]
                         + [(shape, False) for shape in wr.WIDTH_SHAPES])
def test_both_widths_and_a_second_call_give_the_same_bits(sa, shape, sparse):
    x, y = tc.problem(shape[0], shape[1] or sa.wcovariance_max_features(), sparse)
    kw = dict(alpha=0.5, **(dict(nlambda=4, lambda_min_ratio=0.1) if shape[1] is None else wr.WIDTH_PATH), **KW)
    with sa.option("wcovariance_width", 256):
        narrow = sa.sgdnet_wcovariance(x, y, **kw)
    with sa.option("wcovariance_width", 1024):
        wide = sa.sgdnet_wcovariance(x, y, **kw)
    again = sa.sgdnet_wcovariance(x, y, **kw)
    assert (narrow.return_codes == 0).all() and narrow.npasses > 0
    assert same_bits(narrow, wide) and same_bits(narrow, again)
    with sa.option("wcovariance_width", 512):                  # not a width the library has
        with pytest.raises(sa.SgdnetError) as e:
            sa.sgdnet_wcovariance(x, y, **kw)
    assert e.value.code == -1


# ---- (iv) the list converges, and a later screen still adds to it ----

def test_rescreen_input_is_optimal(sa):
    x, y = wr.rescreen_problem()
    fit_and_check(sa, x, y, "re-screen", **wr.RESCREEN)


# ---- (v) lambdas and limits ----

@pytest.mark.parametrize("sparse", [False, True])
def test_user_lambdas_need_not_be_monotone(sa, sparse):
    x, y = tc.problem(300, 199, sparse, seed=1)
    fit = fit_and_check(sa, x, y, ("user lambdas", sparse), alpha=0.5, lambda_=tc.NONMONOTONE)
    assert np.array_equal(fit.lambda_, tc.NONMONOTONE)
    # every lambda's optimum is its own: the same values in decreasing order give the same coefficients
    order = np.argsort(tc.NONMONOTONE)[::-1]
    mono = sa.sgdnet_wcovariance(x, y, alpha=0.5, lambda_=np.array(tc.NONMONOTONE)[order], **KW)
    assert np.abs(fit.beta[:, order] - mono.beta).max() <= 1e-9 * np.abs(mono.beta).max()


def test_max_iter_is_reported(sa):
    x, y = tc.problem(300, 199, False, seed=2)
    fit = sa.sgdnet_wcovariance(x, y, alpha=0.5, nlambda=5, lambda_min_ratio=1e-2, thresh=1e-14, maxit=2)
    done = sa.sgdnet_wcovariance(x, y, alpha=0.5, nlambda=5, lambda_min_ratio=1e-2, thresh=1e-14, maxit=wr.MAXIT)
    # below lambda_max no two sweeps change the coefficients by less than 1e-14 of their size (the restatement needs 15
    # and more at 1e-12 on this shape: test_wcovariance_host.py); with sweeps enough the same path converges
    assert fit.npasses <= 2 * 5 and (fit.return_codes[1:] == 1).all() and (done.return_codes == 0).all()


# ---- (vi) refusals ----

def refused(sa, needle, x, y, **kw):
    with pytest.raises(sa.SgdnetError) as e:
        sa.sgdnet_wcovariance(x, y, **kw)
    assert e.value.code == -5, str(e.value)                   # SGDNET_EUNSUPPORTED
    assert "mode = wcovariance needs" in str(e.value) and needle in str(e.value), str(e.value)


def test_refusals_name_the_condition(sa):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = x[:, 0] + rng.standard_normal(60)
    limit = sa.wcovariance_max_features()
    wide = rng.standard_normal((4, limit + 1))
    refused(sa, "features (limit %d)" % limit, wide, wide[:, 0], nlambda=3)
    refused(sa, "sgdnet_wcovariance_max_features", sp.csc_matrix(wide), wide[:, 0], nlambda=3)
    refused(sa, "family = gaussian", x, (y > 0).astype(float), family="binomial", nlambda=3)
    refused(sa, "family = gaussian", x, np.column_stack([y, -y]), family="mgaussian", nlambda=3)
    refused(sa, "one GPU", x, y, nlambda=3, devices=[0, 0])
    refused(sa, "one GPU", sp.csc_matrix(x), y, nlambda=3, devices=[0, 0])
    refused(sa, "debug = 0", x, y, nlambda=3, debug=True)
    # ... and the mode is reached only by its own entry point: mode = "covariance" still stops at its own limit
    with pytest.raises(sa.SgdnetError, match="mode = covariance needs"):
        sa.sgdnet(rng.standard_normal((20, 199)), rng.standard_normal(20), nlambda=3, mode="covariance")
    assert sa.sgdnet_wcovariance(x, y, nlambda=3).draws_used == 0


# ---- (vii) predict and score on the returned fit, and the R shim ----

def test_predict_and_score_take_the_fit(sa):
    x, y = tc.problem(300, 199, False, seed=4)
    fit = sa.sgdnet_wcovariance(x, y, alpha=0.5, nlambda=4, lambda_min_ratio=1e-2, **KW)
    pred = np.asarray(sa.predict(fit, x))
    assert np.abs(pred - (x @ fit.beta + fit.a0)).max() <= 1e-9 * np.abs(y).max()
    mse = np.asarray(sa.score(fit, x, y, type_measure="mse")).reshape(-1)
    assert np.abs(mse - ((y[:, None] - pred) ** 2).mean(axis=0)).max() <= 1e-9 * (y ** 2).mean()


@pytest.mark.parametrize("sparse", [False, True])
def test_shim_option_gives_the_ctypes_fit(sa, sparse):
    import rshim
    R = rshim.lib()
    R.rmock_reset()
    R.R_init_sgdnet(None)
    n, p, nl = 300, 199, 6
    x, y = tc.problem(n, p, sparse, seed=9)
    rshim.set_option("sgdnet.mode", "wcovariance")
    R.rmock_set_seed(7)
    kw = dict(alpha=0.5, nlambda=nl, lambda_min_ratio=1e-2, thresh=1e-9, maxit=100000)
    ctl = rshim.control_list(family="gaussian", is_sparse=sparse, **kw)
    got = rshim.decode_result(rshim.call("_sgdnet_SgdnetSparse" if sparse else "_sgdnet_SgdnetDense",
                                         rshim.r_dgcmatrix(x) if sparse else rshim.r_matrix(x), rshim.r_matrix(y.reshape(n, 1)), ctl))
    ref = sa.sgdnet_wcovariance(x, y, **kw)
    assert got["unlist_beta"].tobytes() == ref.beta.ravel(order="F").tobytes()
    assert got["a0"][0].tobytes() == ref.a0.tobytes() and got["lambda_"].tobytes() == ref.lambda_.tobytes()
    assert got["dev_ratio"].tobytes() == ref.dev_ratio.tobytes() and got["npasses"] == ref.npasses
    assert R.rmock_unif_count() == 0 and R.rmock_protect_depth() == 0
