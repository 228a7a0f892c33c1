"""sa.sgdnet_wmcovariance (SGDNET_MODE_WMCOVARIANCE, sgdnet_amd/csrc/covariance.hip: cov_wide_group_scale_kernel and
cov_wide_group_path_kernel): the mgaussian path of K responses solved to its optimum with the scaled Gram matrix in global
memory, for up to wmcovariance_max_features(K) features.  Checked against the optimality conditions of the problem the
driver solves (sa.kkt), as tests/test_gpu_mcovariance.py checks sa.sgdnet_mcovariance, and against that mode where both
run.  The shapes sit at the kernels' edges (wmcovariance_reference.SHAPES); tests/test_wmcovariance_host.py runs the numpy
restatement of the algorithm on the same inputs on the CPU.

Seen on an MI355X: worst KKT ratio 2.9e-10 and intercept residual 6.9e-10 lambda (both at the column of mean 1e6; 7e-11
and below elsewhere), coefficients within 1.9e-12 of max|beta| and dev_ratio within 6e-15 of sa.sgdnet_mcovariance's."""
import numpy as np
import pytest
import scipy.sparse as sp

import test_gpu_mcovariance as tm
import wmcovariance_reference as wm

pytestmark = pytest.mark.gpu
KW = dict(thresh=wm.THRESH, maxit=wm.MAXIT)
stacked = tm.stacked


@pytest.fixture(scope="module")
def sa():
    import torch  # noqa: F401
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    return sgdnet_amd


def same_bits(a, b):
    return (stacked(a).tobytes() == stacked(b).tobytes() and a.a0.tobytes() == b.a0.tobytes() and a.dev_ratio.tobytes() == b.dev_ratio.tobytes()
            and a.lambda_.tobytes() == b.lambda_.tobytes() and a.npasses == b.npasses and (a.return_codes == b.return_codes).all())


def fit_and_check(sa, x, y, what, standardize=True, intercept=True, standardize_response=False, **kw):
    fit = sa.sgdnet_wmcovariance(x, y, standardize=standardize, intercept=intercept, standardize_response=standardize_response, **KW, **kw)
    tm.check_fit(sa, fit, x, y, what, standardize, intercept, standardize_response)      # return codes, draws, KKT, dev_ratio
    return fit


# ---- (i) optimality across the envelope ----

def test_limits_are_the_ones_the_host_test_derives(sa):
    for K, limit in wm.LIMITS.items():
        assert sa.wmcovariance_max_features(K) == limit
    assert sa.wmcovariance_max_features(0) == sa.wmcovariance_max_features(4093) == 0
    assert sa.wmcovariance_max_features(2) >= 2048 and sa.wmcovariance_max_features(10) >= 512


@pytest.mark.parametrize("mix", wm.MIXES)
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", wm.SHAPES)
def test_automatic_path_is_optimal(sa, shape, sparse, mix):
    n, p, K = shape
    x, y = wm.problem(n, p, K, sparse)
    nlambda, ratio = wm.path_of(p, mix)
    for intercept, standardize in wm.settings_of(p):
        fit_and_check(sa, x, y, (n, p, K, sparse, mix, intercept, standardize), standardize, intercept, alpha=mix, nlambda=nlambda,
                      lambda_min_ratio=ratio)


@pytest.mark.parametrize("shape", wm.LIMIT_SHAPES)
def test_path_at_the_feature_limit_is_optimal(sa, shape):
    n, K = shape[0], shape[2]
    p = sa.wmcovariance_max_features(K)
    x, y = wm.problem(n, p, K, False)
    fit_and_check(sa, x, y, (n, p, K, "limit"), alpha=0.5, **wm.LIMIT_PATH)


@pytest.mark.parametrize("sparse", [False, True])
def test_standardized_response(sa, sparse):
    x, y = wm.problem(65, 13, 5, sparse, seed=1)
    fit_and_check(sa, x, y, ("standardize_response", sparse), standardize_response=True, alpha=0.5, nlambda=6, lambda_min_ratio=1e-2)


@pytest.mark.parametrize("sparse", [False, True])
def test_large_mean_column_does_not_cancel(sa, sparse):
    x, y = wm.large_mean_problem(sparse)
    fit_and_check(sa, x, y, ("mean 1e6", sparse), alpha=0.5, nlambda=6, lambda_min_ratio=1e-2)


# ---- (ii) the same answer as sa.sgdnet_mcovariance where both run ----

@pytest.mark.parametrize("mix", [0.5, 0.0])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", wm.BOTH_MODES)
def test_same_optimum_as_mcovariance_mode(sa, shape, sparse, mix):
    x, y = wm.problem(*shape, sparse, seed=3)
    kw = dict(alpha=mix, **wm.BOTH_PATH, **KW)
    wide, narrow = sa.sgdnet_wmcovariance(x, y, **kw), sa.sgdnet_mcovariance(x, y, **kw)
    assert (wide.return_codes == 0).all() and (narrow.return_codes == 0).all()
    assert wide.lambda_.tobytes() == narrow.lambda_.tobytes() and wide.nulldev == narrow.nulldev
    scale = np.abs(stacked(narrow)).max()
    rel = np.abs(stacked(wide) - stacked(narrow)).max() / scale
    a0_rel = np.abs(wide.a0 - narrow.a0).max() / scale
    dev = np.abs(wide.dev_ratio - narrow.dev_ratio).max()
    print(shape, sparse, mix, "wide vs mcovariance: coefficients / max|beta| = %.3g, intercepts / max|beta| = %.3g, dev_ratio %.3g" % (rel, a0_rel, dev))
    assert rel <= 10 * wm.BLOCK_CD_REL and a0_rel <= 10 * wm.BLOCK_CD_REL
    assert dev <= 10 * wm.BLOCK_CD_DEV


# ---- (iii) determinism: the workgroup's width, and a second call ----

@pytest.mark.parametrize("shape, sparse", wm.WIDTH_SHAPES)
def test_both_widths_and_a_second_call_give_the_same_bits(sa, shape, sparse):
    n, p, K = shape[0], shape[1] or sa.wmcovariance_max_features(shape[2]), shape[2]
    x, y = wm.problem(n, p, K, sparse)
    kw = dict(alpha=0.5, **(wm.LIMIT_PATH if shape[1] is None else dict(zip(("nlambda", "lambda_min_ratio"), wm.path_of(p, 0.5)))), **KW)
    with sa.option("wmcovariance_width", 256):
        narrow = sa.sgdnet_wmcovariance(x, y, **kw)
    with sa.option("wmcovariance_width", 1024):
        wide = sa.sgdnet_wmcovariance(x, y, **kw)
    again = sa.sgdnet_wmcovariance(x, y, **kw)
    assert (narrow.return_codes == 0).all() and narrow.npasses > 0
    assert same_bits(narrow, wide) and same_bits(narrow, again)
    with sa.option("wmcovariance_width", 512):                 # not a width the library has
        with pytest.raises(sa.SgdnetError) as e:
            sa.sgdnet_wmcovariance(x, y, **kw)
    assert e.value.code == -1


# ---- (iv) the list converges, and a later screen still adds to it ----

def test_rescreen_input_is_optimal(sa):
    x, y = wm.rescreen_problem()
    fit_and_check(sa, x, y, "re-screen", **wm.RESCREEN)


# ---- (v) lambdas and limits ----

@pytest.mark.parametrize("sparse", [False, True])
def test_user_lambdas_need_not_be_monotone(sa, sparse):
    x, y = wm.problem(*wm.NONMONOTONE_SHAPE, sparse, seed=1)
    fit = fit_and_check(sa, x, y, ("user lambdas", sparse), alpha=0.5, lambda_=tm.NONMONOTONE)
    assert np.array_equal(fit.lambda_, tm.NONMONOTONE)
    # every lambda's optimum is its own: the same values in decreasing order give the same coefficients
    order = np.argsort(tm.NONMONOTONE)[::-1]
    mono = sa.sgdnet_wmcovariance(x, y, alpha=0.5, lambda_=np.array(tm.NONMONOTONE)[order], **KW)
    assert np.abs(stacked(fit)[:, :, order] - stacked(mono)).max() <= 1e-9 * np.abs(stacked(mono)).max()


def test_max_iter_is_reported(sa):
    x, y = wm.problem(*wm.NONMONOTONE_SHAPE, False, seed=2)
    kw = dict(alpha=0.5, nlambda=5, lambda_min_ratio=1e-2, thresh=1e-14)
    fit = sa.sgdnet_wmcovariance(x, y, maxit=2, **kw)
    done = sa.sgdnet_wmcovariance(x, y, maxit=wm.MAXIT, **kw)
    # below lambda_max no two sweeps change the coefficients by less than 1e-14 of their size; with sweeps enough the same
    # path converges
    assert fit.npasses <= 2 * 5 and (fit.return_codes[1:] == 1).all() and (done.return_codes == 0).all()


# ---- (vi) refusals ----

def refused(sa, needle, x, y, **kw):
    with pytest.raises(sa.SgdnetError) as e:
        sa.sgdnet_wmcovariance(x, y, **kw)
    assert e.value.code == -5, str(e.value)                   # SGDNET_EUNSUPPORTED
    assert "mode = wmcovariance needs" in str(e.value) and needle in str(e.value), str(e.value)


def test_refusals_name_the_condition(sa):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = np.column_stack([x[:, 0] + rng.standard_normal(60), x[:, 1] - rng.standard_normal(60)])
    limit = sa.wmcovariance_max_features(2)
    wide = rng.standard_normal((4, limit + 1))
    refused(sa, "features (limit %d)" % limit, wide, wide[:, :2], nlambda=3)
    refused(sa, "sgdnet_wmcovariance_max_features(n_classes)", sp.csc_matrix(wide), wide[:, :2], nlambda=3)
    refused(sa, "family = mgaussian", x, y[:, 0], family="gaussian", nlambda=3)
    refused(sa, "family = mgaussian", x, (y[:, 0] > 0).astype(float), family="binomial", nlambda=3)
    refused(sa, "family = mgaussian", x, np.arange(60) % 3, family="multinomial", nlambda=3)
    refused(sa, "one GPU", x, y, nlambda=3, devices=[0, 0])
    refused(sa, "one GPU", sp.csc_matrix(x), y, nlambda=3, devices=[0, 0])
    refused(sa, "debug = 0", x, y, nlambda=3, debug=True)
    # ... and neither mode is the other's fall back: sa.sgdnet_mcovariance still stops at its own limit
    with pytest.raises(sa.SgdnetError, match="mode = mcovariance needs no more features"):
        sa.sgdnet_mcovariance(rng.standard_normal((20, 196)), rng.standard_normal((20, 2)), nlambda=3)
    with pytest.raises(ValueError, match="mode must be one of"):
        sa.sgdnet(x, y, family="mgaussian", nlambda=3, mode="wmcovariance")
    assert sa.sgdnet_wmcovariance(x, y, nlambda=3).draws_used == 0


# ---- (vii) predict and score on the returned fit, and the R shim ----

def test_predict_and_score_take_the_fit(sa):
    x, y = wm.problem(*wm.NONMONOTONE_SHAPE, False, seed=4)
    fit = sa.sgdnet_wmcovariance(x, y, alpha=0.5, nlambda=4, lambda_min_ratio=1e-2, **KW)
    pred = np.asarray(sa.predict(fit, x))
    ref = np.einsum("ij,kjl->ikl", x, stacked(fit)) + fit.a0[None]                    # (n, K, L)
    assert pred.shape == ref.shape and np.abs(pred - ref).max() <= 1e-9 * np.abs(y).max()
    mse = np.asarray(sa.score(fit, x, y, type_measure="mse")).reshape(-1)
    assert mse.shape == (4,) and np.isfinite(mse).all() and (np.diff(mse) < 0).all()     # the training error falls along the path
    rss = ((y[:, :, None] - ref) ** 2).sum(axis=0).mean(axis=0)                       # summed over the samples, the mean of the responses
    assert np.abs(mse - rss).max() <= 1e-9 * rss.max()


@pytest.mark.parametrize("sparse", [False, True])
def test_shim_option_gives_the_ctypes_fit(sa, sparse):
    import rshim
    R = rshim.lib()
    R.rmock_reset()
    R.R_init_sgdnet(None)
    n, p, K, nl = 300, 199, 2, 6
    x, y = wm.problem(n, p, K, sparse, seed=9)
    rshim.set_option("sgdnet.mode", "wmcovariance")
    R.rmock_set_seed(7)
    kw = dict(alpha=0.5, nlambda=nl, lambda_min_ratio=1e-2, thresh=1e-9, maxit=100000)
    ctl = rshim.control_list(family="mgaussian", n_classes=K, is_sparse=sparse, **kw)
    got = rshim.decode_result(rshim.call("_sgdnet_SgdnetSparse" if sparse else "_sgdnet_SgdnetDense",
                                         rshim.r_dgcmatrix(x) if sparse else rshim.r_matrix(x), rshim.r_matrix(y), ctl))
    ref = sa.sgdnet_wmcovariance(x, y, **kw)
    assert got["unlist_beta"].tobytes() == stacked(ref).ravel(order="F").tobytes()
    assert np.asfortranarray(got["a0"]).tobytes(order="F") == np.asfortranarray(ref.a0).tobytes(order="F")
    assert got["lambda_"].tobytes() == ref.lambda_.tobytes()
    assert got["dev_ratio"].tobytes() == ref.dev_ratio.tobytes() and got["npasses"] == ref.npasses
    assert R.rmock_unif_count() == 0 and R.rmock_protect_depth() == 0
