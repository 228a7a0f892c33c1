"""sa.sgdnet_wnewton (SGDNET_MODE_WNEWTON, sgdnet_amd/csrc/newton.hip: wide_scale_kernel and newton_wide_cd_kernel):
the binomial path of one response solved to its optimum by proximal Newton steps with the weighted Gram matrix in global
memory, for up to wnewton_max_features() features.  Checked against the optimality conditions of the problem the driver
solves (sa.kkt), as tests/test_gpu_newton.py checks sa.sgdnet_newton, and against that mode where both run.  The shapes
sit at the kernels' edges (wnewton_reference.SHAPES); tests/test_wnewton_host.py runs the numpy restatement of the
algorithm on the same inputs on the CPU."""
import numpy as np
import pytest
import scipy.sparse as sp

import test_gpu_newton as tn
import wnewton_reference as wr

pytestmark = pytest.mark.gpu
KW = dict(thresh=wr.THRESH)

# Against sa.sgdnet_newton at BOTH_MODES: the bounds sa.sgdnet_wcovariance meets against mode = "covariance".  The numpy
# restatements of the two modes differ by less on the same inputs (test_wnewton_host.py asserts it; measured: at most 3.2e-15
# of max|beta| in the coefficients and the intercept), so these stand.
SAME_OPTIMUM_REL, SAME_DEV_RATIO = 1e-9, 1e-10
# The curvature guard: a wrong H still converges, only in more steps.  Total npasses of the wide mode less
# newton mode's, the two numpy restatements on the same inputs (dense and sparse, mix 0.5 and 0): at most 0
# (test_wnewton_host.py::test_restatements_agree_where_both_modes_run asserts it).  Plus one per lambda.
RESTATEMENT_EXCESS_PASSES = 0


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
    fit = sa.sgdnet_wnewton(x, y, standardize=standardize, intercept=intercept, **KW, **kw)
    assert fit.family == "binomial" and fit.beta.shape[0] == x.shape[1]
    assert (fit.return_codes == 0).all() and fit.draws_used == 0 and np.isfinite(fit.dev_ratio).all(), (what, fit.return_codes)
    tn.assert_optimal(sa.kkt(fit, x, y, standardize=standardize, intercept=intercept), fit.lambda_, what)
    return fit


# ---- (i) optimality across the envelope ----

def test_limit_is_the_one_the_layout_gives(sa):
    assert sa.wnewton_max_features() == wr.LIMIT >= 4096


@pytest.mark.parametrize("mix", wr.MIXES)
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", wr.SHAPES)
def test_automatic_path_is_optimal(sa, shape, sparse, mix):
    n, p = shape[0], shape[1] or sa.wnewton_max_features()
    x, y = tn.problem(n, p, sparse)
    nlambda, ratio = wr.path_of(shape[0], shape[1], mix)
    for intercept, standardize in wr.settings_of(shape[1]):
        fit_and_check(sa, x, y, (n, p, sparse, mix, intercept, standardize), standardize, intercept, alpha=mix, nlambda=nlambda,
                      lambda_min_ratio=ratio)


@pytest.mark.parametrize("sparse", [False, True])
def test_large_mean_column_does_not_cancel(sa, sparse):
    """tests/test_gpu_newton.py's check with its bound: the fit of a column at mean 1e6 is the fit of the same column at
    mean 0, which is optimal."""
    shifted, centred, y = wr.large_mean_twins(sparse)
    a = sa.sgdnet_wnewton(shifted, y, **wr.LARGE_MEAN, **KW)
    b = fit_and_check(sa, centred, y, ("centred twin", sparse), **wr.LARGE_MEAN)
    assert (a.return_codes == 0).all()
    scale = np.abs(b.beta).max()
    print("mean 1e6 vs centred: max coefficient difference / max|beta| = %.3g" % (np.abs(a.beta - b.beta).max() / scale))
    assert np.abs(a.lambda_ - b.lambda_).max() <= wr.LARGE_MEAN_TOL * b.lambda_.max()
    assert np.abs(a.beta - b.beta).max() <= wr.LARGE_MEAN_TOL * scale
    assert np.abs(a.dev_ratio - b.dev_ratio).max() <= wr.LARGE_MEAN_TOL


# ---- (ii) the same answer as sa.sgdnet_newton where both run, in no more passes ----

@pytest.mark.parametrize("mix", [0.5, 0.0])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", wr.BOTH_MODES)
def test_same_optimum_as_newton_mode_in_as_many_passes(sa, shape, sparse, mix):
    x, y = tn.problem(shape[0], shape[1], sparse, seed=3)
    kw = dict(alpha=mix, **wr.BOTH_MODES_PATH, **KW)
    wide, newton = sa.sgdnet_wnewton(x, y, **kw), sa.sgdnet_newton(x, y, **kw)
    assert (wide.return_codes == 0).all() and (newton.return_codes == 0).all()
    # lambda_ and nulldev bit for bit.  A sparse fit of this mode IS the fit of the dense copy (its lambda_max comes from
    # the dense standard deviations), and newton mode's sparse entry rounds its own differently in the last place: the
    # bits to meet are those of the other mode on the matrix this mode fits.
    same_matrix = sa.sgdnet_newton(np.asarray(x.todense()), y, **kw) if sparse else newton
    assert wide.lambda_.tobytes() == same_matrix.lambda_.tobytes() and wide.nulldev == same_matrix.nulldev == newton.nulldev
    scale =np.abs(newton.beta).max()
    print(shape, sparse, mix, "wide vs newton: max coefficient difference / max|beta| = %.3g, dev_ratio %.3g, npasses %g against %g"
          % (max(np.abs(wide.beta - newton.beta).max(), np.abs(wide.a0 - newton.a0).max()) / scale,
             np.abs(wide.dev_ratio - newton.dev_ratio).max(), wide.npasses, newton.npasses))
    assert np.abs(wide.beta - newton.beta).max() <= SAME_OPTIMUM_REL * scale and np.abs(wide.a0 - newton.a0).max() <= SAME_OPTIMUM_REL * scale
    assert np.abs(wide.dev_ratio - newton.dev_ratio).max() <= SAME_DEV_RATIO
    # the curvature guard
    assert wide.npasses <= newton.npasses + RESTATEMENT_EXCESS_PASSES + len(wide.lambda_)


# ---- (iii) determinism: the workgroup's width, a second call, and sparse x ----

@pytest.mark.parametrize("shape, sparse", [((65, 1024), False), ((65, 1024), True), ((63, 14), False), ((63, 14), True), ((40, None), False)]
                         + [(shape, False) for shape in wr.WIDTH_SHAPES])
def test_both_widths_and_a_second_call_give_the_same_bits(sa, shape, sparse):
    x, y = tn.problem(shape[0], shape[1] or sa.wnewton_max_features(), sparse)
    nlambda, ratio = wr.path_of(shape[0], shape[1], 0.5)
    kw = dict(alpha=0.5, nlambda=nlambda, lambda_min_ratio=ratio, **KW)
    with sa.option("wnewton_width", 256):
        narrow = sa.sgdnet_wnewton(x, y, **kw)
    with sa.option("wnewton_width", 1024):
        wide = sa.sgdnet_wnewton(x, y, **kw)
    again = sa.sgdnet_wnewton(x, y, **kw)
    assert (narrow.return_codes == 0).all() and narrow.npasses > 0
    assert same_bits(narrow, wide) and same_bits(narrow, again)
    with sa.option("wnewton_width", 512):                      # not a width the library has
        with pytest.raises(sa.SgdnetError) as e:
            sa.sgdnet_wnewton(x, y, **kw)
    assert e.value.code == -1


@pytest.mark.parametrize("shape", [(65, 15), (300, 199), (65, 256)])
def test_sparse_fit_is_the_dense_fit_of_the_same_matrix(sa, shape):
    x, y = tn.problem(shape[0], shape[1], True)
    kw = dict(alpha=0.5, nlambda=4, lambda_min_ratio=0.1, **KW)
    assert same_bits(sa.sgdnet_wnewton(x, y, **kw), sa.sgdnet_wnewton(np.asarray(x.todense()), y, **kw))
    rng = sa.RRng(3)                                           # a generator handed to the backend comes back as it went
    before = bytes(rng.state)
    fit = wnewton_with(x, y, rng=rng, **kw)
    assert bytes(rng.state) == before and fit.draws_used == 0


# ---- (iv) the list converges inside a solve, and a later screen still adds to it ----

def test_rescreen_input_is_optimal(sa):
    x, y = wr.rescreen_problem()
    fit_and_check(sa, x, y, "re-screen", **wr.RESCREEN)


# ---- (v) lambdas and limits ----

@pytest.mark.parametrize("sparse", [False, True])
def test_user_lambdas_need_not_be_monotone(sa, sparse):
    x, y = tn.problem(300, 199, sparse, seed=1)
    fit = fit_and_check(sa, x, y, ("user lambdas", sparse), alpha=0.5, lambda_=tn.NONMONOTONE)
    assert np.array_equal(fit.lambda_, tn.NONMONOTONE)
    # every lambda's optimum is its own: the same values in decreasing order give the same coefficients
    order = np.argsort(tn.NONMONOTONE)[::-1]
    mono = sa.sgdnet_wnewton(x, y, alpha=0.5, lambda_=np.array(tn.NONMONOTONE)[order], **KW)
    assert np.abs(fit.beta[:, order] - mono.beta).max() <= 1e-9 * np.abs(mono.beta).max()
    assert np.abs(fit.a0[order] - mono.a0).max() <= 1e-9 * max(1.0, np.abs(mono.a0).max())


def test_max_iter_is_reported(sa):
    x, y = tn.problem(300, 199, False, seed=2)
    fit = sa.sgdnet_wnewton(x, y, alpha=0.5, nlambda=5, lambda_min_ratio=1e-2, thresh=1e-14, maxit=2)
    # two Newton steps per lambda do not bring the coefficients to within 1e-14 of their size below lambda_max (the
    # restatement takes 5 and more there: test_wnewton_host.py); one state pass at the start and one per step, more only
    # where a step was halved
    assert (fit.return_codes[1:] == 1).all() and fit.npasses >= 1 + 2 * 4


# ---- (vi) refusals ----

def wnewton_with(x, y, family="binomial", alpha=1, nlambda=100, lambda_min_ratio=None, thresh=1e-3, **over):
    """sgdnet_wnewton's call of the shared front end with arguments sgdnet_wnewton itself does not pass on."""
    from sgdnet_amd import _lib, api
    kw = dict(debug=False, seed=0, rng=None, sample_stream=None, unif=None, mode="wnewton", modes={"wnewton": _lib.MODE_WNEWTON}, batch=0,
              device=0, devices=None)
    kw.update(over)
    return api._fit(x, y, family, alpha, nlambda, lambda_min_ratio, None, 1000, True, True, thresh, False, **kw)


def test_refusals_name_the_condition(sa):
    def refused(needle, x, y, **kw):
        with pytest.raises(sa.SgdnetError) as e:
            wnewton_with(x, y, nlambda=3, **kw)
        assert e.value.code == -5, str(e.value)                   # SGDNET_EUNSUPPORTED
        assert "mode = wnewton needs" in str(e.value) and needle in str(e.value), str(e.value)

    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = x[:, 0] + rng.standard_normal(60)
    cls = (y > 0).astype(float)
    limit = sa.wnewton_max_features()
    wide = rng.standard_normal((4, limit + 1))
    wide_cls = np.array([0.0, 1.0, 0.0, 1.0])
    refused("features (limit %d)" % limit, wide, wide_cls)
    refused("sgdnet_wnewton_max_features", sp.csc_matrix(wide), wide_cls)
    with pytest.raises(sa.SgdnetError, match="mode = wnewton needs no more features"):
        sa.sgdnet_wnewton(wide, wide_cls, nlambda=3)
    refused("family = binomial", x, y, family="gaussian")
    refused("family = binomial", x, np.digitize(y, [-0.5, 0.5]), family="multinomial")
    refused("family = binomial", x, np.column_stack([y, -y]), family="mgaussian")
    refused("one GPU", x, cls, devices=[0, 0])
    refused("one GPU", sp.csc_matrix(x), cls, devices=[0, 0])
    refused("debug = 0", x, cls, debug=True)
    # the dense copy of a sparse x: 70 000 x 2000 x 8 bytes is more than 1 GiB; nothing is stored, so nothing that large is made
    tall = sp.csc_matrix((70_000, 2000))
    tall_cls = (np.arange(70_000) % 2).astype(float)
    refused("the dense copy of a sparse x", tall, tall_cls)
    refused("70000 samples, 2000 features", tall, tall_cls)
    # the mode is reached only by its own entry point: sgdnet() does not know the name, newton mode still stops at its limit
    with pytest.raises(ValueError, match="mode must be one of 'exact', 'batched', 'auto', 'covariance'$"):
        sa.sgdnet(x, cls, family="binomial", nlambda=3, mode="wnewton")
    x199 = rng.standard_normal((20, 199))
    with pytest.raises(sa.SgdnetError, match="mode = newton needs no more features"):
        sa.sgdnet_newton(x199, (x199[:, 0] > 0).astype(float), nlambda=3)
    assert sa.sgdnet(x, cls, family="binomial", nlambda=3, mode="auto").draws_used > 0
    assert sa.sgdnet_wnewton(x, cls, nlambda=3).draws_used == 0


# ---- (vii) predict and score on the returned fit, and the R shim ----

def test_predict_and_score_take_the_fit(sa):
    x, y = tn.problem(300, 199, False, seed=4)
    fit = sa.sgdnet_wnewton(x, y, alpha=0.5, nlambda=4, lambda_min_ratio=1e-2, **KW)
    eta = x @ fit.beta + fit.a0
    link = np.asarray(sa.predict(fit, x)).reshape(eta.shape)
    assert np.abs(link - eta).max() <= 1e-9 * max(1.0, np.abs(eta).max())
    dev = np.asarray(sa.score(fit, x, y, type_measure="deviance")).reshape(-1)
    from sgdnet_amd.score import PROB_MIN
    prob = np.clip(1.0 / (1.0 + np.exp(-eta)), PROB_MIN, 1 - PROB_MIN)
    ref = -2.0 * np.where(y[:, None] == 1.0, np.log(prob), np.log(1 - prob)).mean(axis=0)
    assert dev.shape == ref.shape and np.abs(dev - ref).max() <= 1e-9 * ref.max()


@pytest.mark.parametrize("sparse", [False, True])
def test_shim_option_gives_the_ctypes_fit(sa, sparse):
    import rshim
    R = rshim.lib()
    R.rmock_reset()
    R.R_init_sgdnet(None)
    n, p, nl = 300, 199, 6
    x, y = tn.problem(n, p, sparse, seed=9)
    rshim.set_option("sgdnet.mode", "wnewton")
    R.rmock_set_seed(7)
    kw = dict(alpha=0.5, nlambda=nl, lambda_min_ratio=1e-2, thresh=1e-9, maxit=1000)
    ctl = rshim.control_list(family="binomial", is_sparse=sparse, **kw)
    got = rshim.decode_result(rshim.call("_sgdnet_SgdnetSparse" if sparse else "_sgdnet_SgdnetDense",
                                         rshim.r_dgcmatrix(x) if sparse else rshim.r_matrix(x), rshim.r_matrix(y.reshape(n, 1)), ctl))
    ref = sa.sgdnet_wnewton(x, y, **kw)
    assert got["unlist_beta"].tobytes() == ref.beta.ravel(order="F").tobytes()
    assert got["a0"][0].tobytes() == ref.a0.tobytes() and got["lambda_"].tobytes() == ref.lambda_.tobytes()
    assert got["dev_ratio"].tobytes() == ref.dev_ratio.tobytes() and got["npasses"] == ref.npasses
    assert R.rmock_unif_count() == 0 and R.rmock_protect_depth() == 0
