"""Cross-validation in covariance mode (sgdnet_cv_covariance_*, sgdnet_amd/csrc/covariance.hip), the parts a CPU can check.

pooled_problem() restates in numpy what the device does: per-fold moments of [x - a | y - a_y | 1] about ONE centre a (the
whole-data means), pooled into a training set T (one fold, or the total -- summed in fold order -- minus one) and re-centred
to T's own means t, d = t - a:

    M^T_jk = C^T_jk - d_j s^T_k - d_k s^T_j + n_T d_j d_k

and from it the scaled Gram matrix S and c~ the path kernel iterates on.  direct_problem() forms the same from x[T], y[T]
alone.  The two must agree to rounding: 1e-12 is asserted (the largest difference measured over these cases is printed;
it was 1.8e-14 when the test was written, so the pooling itself stays five orders of magnitude inside the 1e-9 the GPU
tests hold the coefficients to).

The refusals of the native entry points that are decided before a device is looked for, and those of cv_sgdnet(fold_fits=
"batched"), are checked here too: they need no GPU."""
import numpy as np
import pytest

SHAPES = [(37, 2, 3), (195, 15, 3), (192, 17, 3), (1003, 33, 10), (1200, 198, 3)]
POOLING_BOUND = 1e-12


def problem(n, p, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * n + p)
    x = rng.standard_normal((n, p)) * rng.uniform(0.5, 3.0, p) + rng.uniform(-2.0, 2.0, p)
    B = rng.standard_normal(p) * (rng.random(p) < 0.5)
    return x, x @ B + 0.5 * rng.standard_normal(n) + 1.5


def random_folds(n, G, seed=0):
    return np.random.default_rng(seed).permutation(np.arange(n) % G)


def sorted_folds(x, G):
    """folds cut along a sorted column: every fold's mean of that column sits far from the global mean"""
    fold = np.empty(x.shape[0], dtype=np.int64)
    fold[np.argsort(x[:, 0], kind="stable")] = np.arange(x.shape[0]) * G // x.shape[0]
    return fold


def finish(M, nT, p, standardize):
    sd_y = np.sqrt(M[p, p] / nT) or 1.0
    var = np.diag(M)[:p] / nT
    sd = np.where(var > 0, np.sqrt(np.where(var > 0, var, 1.0)), 1.0) if standardize else np.ones(p)
    return M[:p, :p] / nT / np.outer(sd, sd), M[:p, p] / sd_y / nT / sd


def pooled_problem(x, y, fold, G, t, rest, standardize=True, centre=True):
    n, p = x.shape
    a = np.append(x.mean(axis=0) if centre else np.zeros(p), y.mean())
    z = np.column_stack([x, y]) - a
    aug = np.column_stack([z, np.ones(n)])
    Cg = np.array([aug[fold == g].T @ aug[fold == g] for g in range(G)])
    C = Cg[t]
    if rest:
        total = np.zeros_like(C)
        for g in range(G):
            total = total + Cg[g]
        C = total - Cg[t]
    nT, s = C[p + 1, p + 1], C[:p + 1, p + 1]
    d = s / nT
    if not centre:
        d[:p] = 0.0
    M = C[:p + 1, :p + 1] - np.outer(d, s) - np.outer(s, d) + nT * np.outer(d, d)
    return finish(M, nT, p, standardize)


def direct_problem(x, y, standardize=True, centre=True):
    n, p = x.shape
    z = np.column_stack([x - (x.mean(axis=0) if centre else 0.0), y - y.mean()])
    return finish(z.T @ z, float(n), p, standardize)


def test_pooled_moments_are_the_direct_ones():
    worst = 0.0
    for n, p, G in SHAPES:
        x, y = problem(n, p)
        for fold in (random_folds(n, G), sorted_folds(x, G)):
            for rest in (False, True):
                for standardize, centre in ((True, True), (False, True), (False, False)):
                    for t in range(G):
                        T = (fold != t) if rest else (fold == t)
                        S, c = pooled_problem(x, y, fold, G, t, rest, standardize, centre)
                        S0, c0 = direct_problem(x[T], y[T], standardize, centre)
                        err = max(np.abs(S - S0).max() / np.abs(S0).max(), np.abs(c - c0).max() / max(np.abs(c0).max(), 1e-300))
                        worst = max(worst, err)
                        assert err <= POOLING_BOUND, (n, p, G, rest, standardize, centre, t, err)
    print("pooled vs direct S / c~: largest relative difference %.3g" % worst)


def test_pooling_with_a_large_mean_column_does_not_cancel():
    """a column of mean 1e6 and sd 1: deviations are taken from the whole-data mean BEFORE anything is multiplied, so the
    correction s s' / n_T is of the order of the column's variance, not of its squared mean.  What is left is the rounding of
    the stored entries themselves (1e6 * 2^-53 = 1.2e-10 absolute on deviations of order 1), which x[T] suffers as well."""
    n, p, G = 195, 15, 3
    x, y = problem(n, p, seed=1)
    x[:, 3] = 1e6 + np.random.default_rng(5).standard_normal(n)
    for fold in (random_folds(n, G), sorted_folds(x[:, [3]], G)):
        for rest in (False, True):
            for t in range(G):
                T = (fold != t) if rest else (fold == t)
                S, c = pooled_problem(x, y, fold, G, t, rest)
                S0, c0 = direct_problem(x[T], y[T])
                assert np.abs(S - S0).max() <= 1e-8 and np.abs(c - c0).max() <= 1e-8


# ---- refusals that need no device ----

def native_refusal(code, needle, x, y, foldid, alpha=0.5, lam=(0.1, 0.01), **kw):
    import sgdnet_amd as sa
    with pytest.raises(sa.SgdnetError) as e:
        sa.cv_covariance_fits(x, y, foldid, alpha, np.asarray(lam, dtype=float), **kw)
    assert e.value.code == code and needle in str(e.value), str(e.value)


def test_native_refusals_name_the_condition():
    import ctypes as C

    import scipy.sparse as sp

    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = x[:, 0] + rng.standard_normal(60)
    fold = np.arange(60) % 3
    wide = rng.standard_normal((30, sa.covariance_max_features() + 1))
    native_refusal(-5, "mode = covariance needs no more features than sgdnet_covariance_max_features()", wide, wide[:, 0], np.arange(30) % 3)
    native_refusal(-5, "mode = covariance needs no more features", sp.csc_matrix(wide), wide[:, 0], np.arange(30) % 3)
    # leave-one-out at 198 features fits the 64 MiB of group moments up to 209 rows
    big = rng.standard_normal((300, sa.covariance_max_features()))
    native_refusal(-5, "mode = covariance needs the group moments within", big, big[:, 0], np.arange(300))

    # what cv_covariance_fits cannot express goes through the C ABI directly
    L = sa.load()
    xf, yf, f32 = np.asfortranarray(x), np.ascontiguousarray(y), np.ascontiguousarray(fold, dtype=np.int32)
    alphas, lam = np.array([0.5]), np.array([[0.1, 0.01]])

    def call(fold_arr=f32, n_groups=3, lam_arr=lam, **ctl_fields):
        ctl = _lib.Control()
        ctl.family, ctl.intercept, ctl.standardize, ctl.max_iter, ctl.tol, ctl.n_lambda, ctl.n_classes = 0, 1, 1, 100, 1e-7, 2, 1
        for k, v in ctl_fields.items():
            setattr(ctl, k, v)
        out = [np.zeros(3 * 2), np.zeros(3 * 2 * 4), np.zeros(3 * 2), np.zeros(3 * 2), np.zeros(3), np.zeros(3)]
        res = _lib.CvCovResult(*[_lib.dptr(a) for a in out])
        rc = L.sgdnet_cv_covariance_dense(_lib.dptr(xf), 60, 4, _lib.dptr(yf), fold_arr.ctypes.data_as(C.POINTER(C.c_int32)), n_groups, 0,
                                          C.byref(ctl), 1, _lib.dptr(alphas), _lib.dptr(lam_arr), C.byref(res))
        return rc, L.sgdnet_last_error().decode()

    rc, msg = call(n_gpus=2)
    assert rc == -5 and msg.startswith("mode = covariance needs one GPU"), msg
    rc, msg = call(debug=1)
    assert rc == -5 and msg.startswith("mode = covariance needs debug = 0"), msg
    rc, msg = call(family=1)
    assert rc == -5 and msg.startswith("mode = covariance needs family = gaussian"), msg
    bad = f32.copy()
    bad[7] = 3
    rc, msg = call(fold_arr=bad)
    assert rc == -1 and "fold[7] = 3" in msg, msg
    bad[7] = -1
    rc, msg = call(fold_arr=bad)
    assert rc == -1 and "fold[7] = -1" in msg, msg
    rc, msg = call(n_groups=4)
    assert rc == -1 and "group 3 of 4 is empty" in msg, msg
    rc, msg = call(lam_arr=np.array([[0.1, -0.01]]))
    assert rc == -1 and "negative" in msg, msg


def test_python_refusals_name_the_condition():
    import sgdnet_amd as sa
    assert "cv_covariance_fits" in sa.__all__
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = x[:, 0] + rng.standard_normal(60)
    for needle, kw in (("mode='covariance'", dict()), ("mode='covariance'", dict(mode="auto")),
                       ("family='gaussian'", dict(mode="covariance", family="binomial")),
                       ("one device", dict(mode="covariance", devices=[0, 1])),
                       ("debug", dict(mode="covariance", debug=True)),
                       ("'separate' or 'batched'", dict(mode="covariance", fold_fits="fused"))):
        kw.setdefault("fold_fits", "batched")
        with pytest.raises(ValueError) as e:
            sa.cv_sgdnet(x, (y > 0).astype(float) if kw.get("family") == "binomial" else y, nfolds=3, **kw)
        assert needle in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        sa.cv_covariance_fits(x, y, np.arange(60) % 3, [0.5, 1.0], [[0.1, 0.01]])            # one lambda array per alpha
    with pytest.raises(ValueError):
        sa.cv_covariance_fits(x, y, np.arange(60) % 3, 0.5, [0.1, -0.01])
    with pytest.raises(ValueError):
        sa.cv_covariance_fits(x, y, np.arange(60) % 3, 0.5, [0.1], train_on="others")
