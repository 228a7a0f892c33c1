"""sa.sgdnet_wmnewton (SGDNET_MODE_WMNEWTON, sgdnet_amd/csrc/mnewton.hip: mnewton_wide_scale_kernel and
mnewton_wide_cd_kernel): the multinomial path solved to its optimum by proximal Newton steps with the joint Hessian of all
Q = K (p + 1) coordinates in global memory, for up to wmnewton_max_features(K) features.  Checked against the optimality
conditions of the problem the driver solves (sa.kkt), as tests/test_gpu_mnewton.py checks sa.sgdnet_mnewton, and against
that mode where both run.  The shapes sit at the kernels' edges (wmnewton_reference.SHAPES);
tests/test_wmnewton_host.py runs the numpy restatement of the algorithm on the same inputs on the CPU.

At mix = 1 and an even K the optimum need not be unique in the coefficients (test_gpu_mnewton.py): there only the
certificate and the deviance are compared, never coefficients."""
import numpy as np
import pytest
import scipy.sparse as sp

import test_gpu_mnewton as tm
import wmnewton_reference as wr

pytestmark = pytest.mark.gpu
KW = dict(thresh=wr.THRESH)
stacked, centred = tm.stacked, tm.centred

# Against sa.sgdnet_mnewton at BOTH_MODES: the bounds sa.sgdnet_wnewton meets against sa.sgdnet_newton
# (tests/test_gpu_wnewton.py).  The numpy restatements of the two modes differ by less on the same inputs
# (test_wmnewton_host.py::test_restatements_agree_where_both_modes_run asserts these same bounds), so they stand.
SAME_OPTIMUM_REL, SAME_DEV_RATIO = 1e-9, 1e-10
# The curvature guard: a wrong H still converges, only in more steps.  Total npasses of the wide mode less mnewton mode's,
# the two numpy restatements on the same inputs: at most 0 (test_wmnewton_host.py asserts it).  Plus one per lambda.
RESTATEMENT_EXCESS_PASSES = 0


@pytest.fixture(scope="module")
def sa():
    import torch  # noqa: F401
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    return sgdnet_amd


def same_bits(a, b):
    return (stacked(a).tobytes() == stacked(b).tobytes() and np.asarray(a.a0).tobytes() == np.asarray(b.a0).tobytes()
            and a.dev_ratio.tobytes() == b.dev_ratio.tobytes() and a.lambda_.tobytes() == b.lambda_.tobytes() and a.npasses == b.npasses
            and (a.return_codes == b.return_codes).all())


def fit_and_check(sa, x, y, what, standardize=True, intercept=True, **kw):
    fit = sa.sgdnet_wmnewton(x, y, standardize=standardize, intercept=intercept, **KW, **kw)
    tm.check_fit(sa, fit, x, y, what, standardize, intercept)      # return codes 0, draws_used 0, finite dev_ratio, KKT_BOUND
    return fit


def shape_problem(shape, sparse=False, seed=0):
    return wr.problem(shape[0], wr.features_of(shape), shape[2], sparse=sparse, seed=seed)


# ---- (i) the limit, and optimality across the envelope ----

def test_limit_is_the_one_the_layout_gives(sa):
    assert [sa.wmnewton_max_features(K) for K in wr.LIMIT_KS] == [wr.max_features(K) for K in wr.LIMIT_KS]
    for K, p in wr.LIMIT_TABLE.items():
        assert sa.wmnewton_max_features(K) == p


@pytest.mark.parametrize("mix", wr.MIXES)
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", wr.SHAPES)
def test_automatic_path_is_optimal(sa, shape, sparse, mix):
    x, y = shape_problem(shape, sparse)
    K, p = shape[2], wr.features_of(shape)
    nlambda, ratio = wr.path_of(shape, mix)
    for intercept, standardize in wr.settings_of(shape):
        fit = fit_and_check(sa, x, y, (shape, sparse, mix, intercept, standardize), standardize, intercept, alpha=mix, nlambda=nlambda,
                            lambda_min_ratio=ratio)
        assert len(fit.beta) == K and fit.beta[0].shape == (p, nlambda)


# ---- (ii) the same answer as sa.sgdnet_mnewton where both run, in no more passes ----

@pytest.mark.parametrize("mix", wr.MIXES)
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("shape", wr.BOTH_MODES)
def test_same_optimum_as_mnewton_mode_in_as_many_passes(sa, shape, sparse, mix):
    x, y = shape_problem(shape, sparse)
    K = shape[2]
    nlambda, ratio = wr.path_of(shape, mix)
    kw = dict(alpha=mix, nlambda=nlambda, lambda_min_ratio=ratio, **KW)
    wide, narrow = sa.sgdnet_wmnewton(x, y, **kw), sa.sgdnet_mnewton(x, y, **kw)
    assert (wide.return_codes == 0).all() and (narrow.return_codes == 0).all()
    assert wide.lambda_.tobytes() == narrow.lambda_.tobytes() and wide.nulldev == narrow.nulldev
    scale = np.abs(stacked(narrow)).max()
    coef = np.abs(stacked(wide) - stacked(narrow)).max() / scale
    icpt = np.abs(np.asarray(wide.a0) - np.asarray(narrow.a0)).max() / scale
    ddev = np.abs(wide.dev_ratio - narrow.dev_ratio).max()
    print(shape, sparse, mix, "wide vs mnewton: coefficients %.3g intercepts %.3g of max|beta|, dev_ratio %.3g, npasses %g against %g"
          % (coef, icpt, ddev, wide.npasses, narrow.npasses))
    if mix < 1 or K % 2 == 1:                                      # (where the optimum is unique in the coefficients)
        assert coef <= SAME_OPTIMUM_REL and icpt <= SAME_OPTIMUM_REL
    assert ddev <= SAME_DEV_RATIO
    # the curvature guard
    assert wide.npasses <= narrow.npasses + RESTATEMENT_EXCESS_PASSES + len(wide.lambda_)


@pytest.fixture(scope="module")
def restated_passes():
    """the restatement's state passes on PASS_GUARD_SHAPES (mix 0.5, the default setting), computed once"""
    out = {}
    for shape in wr.PASS_GUARD_SHAPES:
        x, y = shape_problem(shape)
        nlambda, ratio = wr.path_of(shape, 0.5)
        lam = wr.automatic_lambdas(x, y, shape[2], 0.5, True, nlambda, ratio)
        _, _, _, info = wr.numpy_wide_mnewton_path(x, y, shape[2], lam, 0.5)
        assert info["codes"] == [0] * nlambda
        out[shape] = info["passes"]
    return out


@pytest.mark.parametrize("shape", wr.PASS_GUARD_SHAPES)
def test_no_more_passes_than_the_restatement_beyond_mnewtons_limit(sa, restated_passes, shape):
    """the curvature guard where mode = mnewton does not run: the restatement's own pass count"""
    x, y = shape_problem(shape)
    nlambda, ratio = wr.path_of(shape, 0.5)
    fit = fit_and_check(sa, x, y, ("pass guard", shape), alpha=0.5, nlambda=nlambda, lambda_min_ratio=ratio)
    print(shape, "npasses %g against the restatement's %d" % (fit.npasses, restated_passes[shape]))
    assert fit.npasses <= restated_passes[shape] + RESTATEMENT_EXCESS_PASSES + nlambda


# ---- (iii) determinism: the workgroup's width, a second call, and sparse x ----

@pytest.mark.parametrize("shape", wr.SHAPES)
def test_both_widths_and_a_second_call_give_the_same_bits(sa, shape):
    x, y = shape_problem(shape)
    # (at the limit two lambdas: the 256-lane solve of 5820 coordinates is the slow one, and three fits run here)
    nlambda, ratio = (2, 0.5) if shape[1] is None else wr.path_of(shape, 0.5)
    kw = dict(alpha=0.5, nlambda=nlambda, lambda_min_ratio=ratio, **KW)
    with sa.option("wmnewton_width", 256):
        narrow = sa.sgdnet_wmnewton(x, y, **kw)
    with sa.option("wmnewton_width", 1024):
        wide = sa.sgdnet_wmnewton(x, y, **kw)
    again = sa.sgdnet_wmnewton(x, y, **kw)
    assert (narrow.return_codes == 0).all() and narrow.npasses > 0
    assert same_bits(narrow, wide) and same_bits(narrow, again)


def test_a_width_the_library_has_not_is_refused(sa):
    x, y = shape_problem((90, 13, 3))
    with sa.option("wmnewton_width", 512):
        with pytest.raises(sa.SgdnetError) as e:
            sa.sgdnet_wmnewton(x, y, nlambda=3)
    assert e.value.code == -1


@pytest.mark.parametrize("shape", wr.BEYOND_MNEWTON + wr.ODD_Q + wr.MANY_CLASSES[:1] + wr.TILE_SHAPES[1:2] + wr.LIMIT_SHAPES[1:2])
def test_sparse_fit_is_the_dense_fit_of_the_same_matrix(sa, shape):
    xs, y = shape_problem(shape, sparse=True)
    assert sp.issparse(xs)
    nlambda, ratio = wr.path_of(shape, 0.5)
    for intercept, standardize in wr.settings_of(shape):
        kw = dict(alpha=0.5, nlambda=nlambda, lambda_min_ratio=ratio, intercept=intercept, standardize=standardize, **KW)
        a, b = sa.sgdnet_wmnewton(xs, y, **kw), sa.sgdnet_wmnewton(xs.toarray(), y, **kw)
        assert same_bits(a, b) and a.nulldev == b.nulldev and (a.return_codes == 0).all() and a.draws_used == 0
    rng = sa.RRng(3)                                           # a generator handed to the backend comes back as it went
    before = bytes(rng.state)
    fit = wmnewton_with(xs, y, rng=rng, nlambda=3)
    assert bytes(rng.state) == before and fit.draws_used == 0


def test_sparse_entries_stored_twice_add_up(sa):
    xs, y = shape_problem((90, 66, 3), sparse=True)
    xs = sp.csc_matrix(xs)
    xs.sort_indices()
    # every entry stored as two halves next to each other (the three-array form keeps them apart): v / 2 + v / 2 == v exactly,
    # so the dense copy, and with it the fit, is the same bit for bit
    twice = sp.csc_matrix((np.repeat(0.5 * xs.data, 2), np.repeat(xs.indices, 2), 2 * xs.indptr), shape=xs.shape)
    assert twice.nnz == 2 * xs.nnz and not twice.has_canonical_format
    kw = dict(alpha=0.5, nlambda=4, lambda_min_ratio=0.1, **KW)
    a, b = sa.sgdnet_wmnewton(twice, y, **kw), sa.sgdnet_wmnewton(xs, y, **kw)
    assert (a.return_codes == 0).all() and same_bits(a, b)


# ---- (iv) lambdas and limits ----

def test_lambda_max_first(sa):
    """The automatic path starts at lambda_max: all coefficients exactly zero there, the intercepts at the null model."""
    x, y = tm.iris()
    for intercept, standardize in wr.ALL_SETTINGS:
        for mix in (1.0, 0.5):
            fit = sa.sgdnet_wmnewton(x, y, alpha=mix, nlambda=4, intercept=intercept, standardize=standardize, **KW)
            assert (stacked(fit)[:, :, 0] == 0.0).all(), (intercept, standardize, mix, stacked(fit)[:, :, 0])
            assert np.abs(np.asarray(fit.a0)[:, 0] - tm.null_intercepts(y, 3, intercept)).max() <= 1e-12
            assert abs(fit.dev_ratio[0]) <= 1e-12 and fit.return_codes[0] == 0
    x, y = shape_problem((90, 66, 3))                               # beyond mnewton's limit; classes of different sizes
    fit = sa.sgdnet_wmnewton(x, y, alpha=1.0, nlambda=4, lambda_min_ratio=0.1, **KW)
    assert (stacked(fit)[:, :, 0] == 0.0).all()
    assert np.abs(np.asarray(fit.a0)[:, 0] - tm.null_intercepts(y, 3, True)).max() <= 1e-12


def test_user_lambdas_need_not_be_monotone(sa):
    x, y = wr.problem(200, 6, 5, seed=2)
    fit = fit_and_check(sa, x, y, "user lambdas", alpha=0.5, lambda_=tm.NONMONOTONE)
    assert np.array_equal(fit.lambda_, tm.NONMONOTONE)
    # every lambda's optimum is its own (unique at mix 0.5): the same values in decreasing order give the same coefficients
    order = np.argsort(tm.NONMONOTONE)[::-1]
    mono = sa.sgdnet_wmnewton(x, y, alpha=0.5, lambda_=np.array(tm.NONMONOTONE)[order], **KW)
    assert np.abs(stacked(fit)[:, :, order] - stacked(mono)).max() <= 1e-9 * np.abs(stacked(mono)).max()


def test_max_iter_is_reported(sa):
    x, y = wr.problem(200, 6, 5, seed=3)
    fit = sa.sgdnet_wmnewton(x, y, alpha=0.5, nlambda=5, lambda_min_ratio=1e-2, thresh=1e-14, maxit=1)
    assert (fit.return_codes[1:] == 1).all() and np.isfinite(stacked(fit)).all() and np.isfinite(fit.dev_ratio).all()
    assert 1 + 4 <= fit.npasses <= 1 + 5 * (1 + wr.MAX_HALVINGS)


# ---- (v) degenerate inputs ----

def test_constant_column(sa):
    x, y = wr.problem(160, 5, 4, seed=5)
    x[:, 2] = 3.0
    for mix in wr.MIXES:
        for standardize in (True, False):
            fit = fit_and_check(sa, x, y, ("constant column", mix, standardize), standardize=standardize, alpha=mix, nlambda=5,
                                lambda_min_ratio=1e-2)
            assert (stacked(fit)[:, 2] == 0.0).all() and np.isfinite(stacked(fit)).all()


def native_fit(sa, x, y, K, alpha, nlambda, lambda_min_ratio, thresh, maxit=1000):
    """SGDNET_MODE_WMNEWTON through the native entry point on class codes, without sgdnet()'s checks of the response."""
    import ctypes as C
    from types import SimpleNamespace
    from sgdnet_amd import _lib
    n, p = x.shape
    xf, ym = np.asfortranarray(x, dtype=np.float64), np.asfortranarray(y.reshape(-1, 1), dtype=np.float64)
    ctl = _lib.Control()
    ctl.elasticnet_mix, ctl.family, ctl.intercept, ctl.standardize = float(alpha), _lib.FAMILIES["multinomial"], 1, 1
    ctl.lambda_min_ratio, ctl.max_iter, ctl.n_lambda, ctl.n_classes, ctl.tol = lambda_min_ratio, maxit, nlambda, K, thresh
    ctl.mode = _lib.MODE_WMNEWTON
    a0, beta = np.zeros((K, nlambda), order="F"), np.zeros((K, p, nlambda), order="F")
    lam, dev, codes = np.zeros(nlambda), np.zeros(nlambda), np.zeros(nlambda)
    res = _lib.Result()
    res.a0, res.beta, res.lambda_ = _lib.dptr(a0), _lib.dptr(beta), _lib.dptr(lam)
    res.dev_ratio, res.return_codes = _lib.dptr(dev), _lib.dptr(codes)
    _lib.check(_lib.load().sgdnet_fit_dense(_lib.dptr(xf), n, p, _lib.dptr(ym), 1, C.byref(ctl), C.byref(res)))
    return SimpleNamespace(a0=a0 - a0.mean(axis=0, keepdims=True), beta=[beta[k] for k in range(K)], lambda_=lam, dev_ratio=dev,
                           return_codes=codes, draws_used=res.draws_used, npasses=res.npasses, alpha=alpha, family="multinomial")


def test_class_with_a_single_member(sa):
    """sgdnet()'s validation refuses such a response; the backend takes it (the R front end's check is not the shim's)."""
    x, y = wr.problem(120, 4, 3, seed=6)
    y[y == 2] = 1.0
    y[7] = 2.0
    assert (y == 2).sum() == 1
    with pytest.raises(ValueError, match="one class only has 1 observations"):
        sa.sgdnet_wmnewton(x, y, nlambda=3)
    fit = native_fit(sa, x, y, 3, alpha=0.5, nlambda=5, lambda_min_ratio=1e-2, thresh=wr.THRESH)
    tm.check_fit(sa, fit, x, y, "single member")


# ---- (vi) refusals and dispatch ----

def wmnewton_with(x, y, family="multinomial", alpha=0.5, nlambda=3, lambda_min_ratio=None, thresh=1e-3, lambda_=None, **over):
    """sgdnet_wmnewton's call of the shared front end with arguments sgdnet_wmnewton itself does not pass on."""
    from sgdnet_amd import _lib, api
    kw = dict(debug=False, seed=0, rng=None, sample_stream=None, unif=None, batch=0, device=0, devices=None)
    kw.update(over)
    return api._fit(x, y, family, alpha, nlambda, lambda_min_ratio, lambda_, 1000, True, True, thresh, False, mode="wmnewton",
                    modes={"wmnewton": _lib.MODE_WMNEWTON}, min_classes=2, **kw)


def refused(sa, needle, x, y, **kw):
    with pytest.raises(sa.SgdnetError) as e:
        wmnewton_with(x, y, **kw)
    assert e.value.code == -5, str(e.value)                   # SGDNET_EUNSUPPORTED
    assert "mode = wmnewton needs " in str(e.value) and needle in str(e.value), str(e.value)


def test_refusals_name_the_condition(sa):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = np.arange(60) % 3
    refused(sa, "family = multinomial", x, (y > 0).astype(float), family="binomial")
    refused(sa, "family = multinomial", x, x[:, 0] + rng.standard_normal(60), family="gaussian")
    for K in (2, 3):
        limit = sa.wmnewton_max_features(K)
        wide, yk = rng.standard_normal((40, limit + 1)), np.arange(40) % K
        refused(sa, "features (limit %d)" % limit, wide, yk)
        refused(sa, "sgdnet_wmnewton_max_features(n_classes)", sp.csc_matrix(wide), yk)
    refused(sa, "one GPU", x, y, devices=[0, 0])
    refused(sa, "one GPU", sp.csc_matrix(x), y, devices=[0, 0])
    refused(sa, "debug = 0", x, y, debug=True)
    # the dense copy of a sparse x: 70 000 x 2000 x 8 bytes is more than 1 GiB; nothing is stored, so nothing that large is made
    tall = sp.csc_matrix((70_000, 2000))
    tall_cls = (np.arange(70_000) % 2).astype(float)
    refused(sa, "the dense copy of a sparse x", tall, tall_cls, lambda_=[0.1, 0.05], nlambda=2)
    refused(sa, "70000 samples, 2000 features", tall, tall_cls, lambda_=[0.1, 0.05], nlambda=2)


def test_the_other_doors_stay_shut(sa):
    """No silent fall back: the other modes still refuse multinomial, mnewton still stops at its own limit, sgdnet() does
    not know the name and auto still draws."""
    x, y = tm.iris()
    with pytest.raises(ValueError, match="mode must be one of 'exact', 'batched', 'auto', 'covariance'$"):
        sa.sgdnet(x, y, family="multinomial", nlambda=3, mode="wmnewton")
    with pytest.raises(sa.SgdnetError) as e:
        sa.sgdnet(x, y, family="multinomial", nlambda=3, mode="covariance")
    assert e.value.code == -5 and "mode = covariance needs family = gaussian" in str(e.value)
    from sgdnet_amd import _lib, api
    for name, code, needle in (("newton", _lib.MODE_NEWTON, "mode = newton needs family = binomial"),
                               ("wnewton", _lib.MODE_WNEWTON, "mode = wnewton needs family = binomial"),
                               ("mcovariance", _lib.MODE_MCOVARIANCE, "mode = mcovariance needs family = mgaussian"),
                               ("wcovariance", _lib.MODE_WCOVARIANCE, "mode = wcovariance needs family = gaussian"),
                               ("wmcovariance", _lib.MODE_WMCOVARIANCE, "mode = wmcovariance needs family = mgaussian")):
        with pytest.raises(sa.SgdnetError) as e:
            api._fit(x, y, "multinomial", 0.5, 3, None, None, 1000, True, True, 1e-3, False, debug=False, seed=0, rng=None,
                     sample_stream=None, unif=None, mode=name, modes={name: code}, batch=0, device=0, devices=None)
        assert e.value.code == -5 and needle in str(e.value)
    for K in (2, 3, 10):
        wide, yk = np.random.default_rng(K).standard_normal((40, tm.pmax(K) + 1)), np.arange(40) % K
        with pytest.raises(sa.SgdnetError, match="mode = mnewton needs no more features"):
            sa.sgdnet_mnewton(wide, yk, nlambda=3)
        assert sa.sgdnet_wmnewton(wide, yk, nlambda=3, lambda_min_ratio=0.5).draws_used == 0     # ... which this mode takes
    assert sa.sgdnet(x, y, family="multinomial", alpha=0.8, nlambda=5, mode="auto", seed=1).draws_used > 0
    assert sa.sgdnet_wmnewton(x, y, alpha=0.8, nlambda=5).draws_used == 0


# ---- (vii) the R shim ----

@pytest.mark.parametrize("sparse", [False, True])
def test_shim_option_gives_the_ctypes_fit(sa, sparse):
    import rshim
    R = rshim.lib()
    R.rmock_reset()
    R.R_init_sgdnet(None)
    n, p, K, nl = 90, 66, 3, 4
    x, y = wr.problem(n, p, K, sparse=sparse, seed=12)
    rshim.set_option("sgdnet.mode", "wmnewton")
    R.rmock_set_seed(7)
    kw = dict(alpha=0.5, nlambda=nl, lambda_min_ratio=0.1, thresh=1e-9, maxit=1000)
    ctl = rshim.control_list(family="multinomial", n_classes=K, is_sparse=sparse, **kw)
    got = rshim.decode_result(rshim.call("_sgdnet_SgdnetSparse" if sparse else "_sgdnet_SgdnetDense",
                                         rshim.r_dgcmatrix(x) if sparse else rshim.r_matrix(x), rshim.r_matrix(y.reshape(-1, 1)), ctl))
    ref = wmnewton_with(x, y, **{k: v for k, v in kw.items() if k != "maxit"})
    assert got["unlist_beta"].tobytes() == stacked(ref).ravel(order="F").tobytes()
    # the shim returns the backend's intercepts (class mean removed there); sgdnet() removes the class mean once more
    assert np.abs(centred(got["a0"]) - np.asarray(ref.a0)).max() <= 1e-15 * max(1.0, np.abs(ref.a0).max())
    assert got["lambda_"].tobytes() == ref.lambda_.tobytes()
    assert got["dev_ratio"].tobytes() == ref.dev_ratio.tobytes() and got["npasses"] == ref.npasses
    assert R.rmock_unif_count() == 0 and R.rmock_protect_depth() == 0
