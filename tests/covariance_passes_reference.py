"""Pure-numpy reference of the stages of the covariance family (sgdnet_amd/csrc/covariance.hip, moments_device.hpp), shared by
tests/test_covariance_passes_reference.py (CPU) and tests/test_gpu_covariance_passes.py / tests/test_gpu_cv_covariance_passes.py
(GPU): the long-double truth of every stage, a rounding-error bound on |computed - truth| composed over the kernel's own
arithmetic, float64 restatements of the kernels (with the wrong versions the checks must reject), and the inputs.

The error model (`Val`, fl_*, gamma: u = 2^-53, one rounding per operation, a sum of m terms in ANY order errs by at most
gamma_m sum|t_i|) is tests/setup_reference.py's and the summation orders are tests/newton_reference.py's: imported, not
copied.  Every stage is checked in isolation: its truth is formed from what the stage BEFORE it returned, so a failure names
one kernel.  No tolerance in this file comes from what a device returned.

means      cov_sum_kernel, cov_response_centre_kernel: the sum of the stored values (dense: all) over n, exactly 0 without
           centring; the response sums bounded over n terms; the response means one IEEE division of the returned sum (bitwise).
dense      cov_dense_tile_kernel + cov_reduce_kernel: entry (a, b) = sum_i fl(fl(x_ia - c_a) fl(x_ib - c_b)) about the RETURNED
           centres: the roundings of both deviations and of the product, then gamma_(n+2) sum|terms| for the any-order sum
           (64-row steps, chunks in order).  Bitwise: M == M', the corner n_g.
sparse     cov_sparse_pair_kernel: the kernel adds
               both = sum_{J and K} fl(d_j d_k), only_j = sum_{J \\ K} d_j, only_k = sum_{K \\ J} d_k, counts,
               C_jk = ((both - m_k only_j) - m_j only_k) + ((n_g - |J or K|) m_j) m_k
           the response columns  sum_J fl(d_j y~) - m_j (s_y - sum_J y~)  (one fit: 0 for the bracket of a full column), the ones
           column  sum_J d_j - (n_g - |J|) m_j, and cov_group_response(s)_kernel the response block.  The truth is that identity
           in long double with the RETURNED n_g and response sums, the bound composed over THOSE terms.
total      cov_total_kernel: G terms, against the returned Mg.
assembly   cov_assemble_kernel, mcov_assemble_kernel, wcov_cv_stats_kernel + wcov_cv_assemble_kernel, wmcov_cv_stats_kernel +
           wmcov_cv_assemble_kernel, from the returned Mg and total:
               C = total - group (rest), n_T its corner, s = its last column, d = s / n_T (0 where not centred),
               M^T_jk = ((C_jk - d_j s_k) - d_k s_j) + (n_T d_j) d_k,   sd = sqrt(M^T_jj / n_T)
           composed step by step (fl_sub, fl_mul, fl_div, fl_sqrt).  The same composition run on the moment stage's own
           reference (value AND bound) instead of the returned matrices gives the bound of the whole chain, inside which the
           outputs are compared with the long-double moments of x[T], y[T] formed directly.
constant   DESIGN.md 4.5: a column (feature or response) is judged constant on T when its re-centred square q is not above
               tol = (n_T + G_summed + 8) 2^-52 (A_C + 2 |d| A_s + n_T d^2)
           A_C = |C_jj| (rest: |total_jj| + |group_jj|), A_s likewise of the sums, G_summed = G with rest and 0 without:
           the rounding bound of the re-centring expression for a column whose deviations on T are all the same double
           (derivation in DESIGN.md).  Such a column gets scale 1 and exact zeros in what the path kernel reads.
           constant_margin() asserts that every exactly-constant column falls under the rule and reports how far the others are.
scale      wide_scale_kernel / cov_wide_group_scale_kernel and the narrow path kernels' c: divisions only, restated bit for bit."""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import newton_reference as N
from newton_reference import SUMS, seq_sum
from setup_reference import LD, U, Val, fl_add, fl_div, fl_mul, fl_sqrt, fl_sub, fl_sum, gamma

assert fl_sum and gamma     # (the error model in use: fl_sum for the short sums, gamma through _gam for the matrix forms)

TILE_COLS, TILE_ROWS = 16, 64
COV_MAX_FEATURES = 198      # csrc/covariance.hpp: kCovMaxFeatures (the GPU tests assert the library agrees)
EPS = 2.0 ** -52


def mcov_max_features(K):
    p = 1
    while (p + 1) * (p + 2) // 2 + 3 * (p + 1) * K <= 20480:
        p += 1
    return p


def wide_leading_dim(p):
    return (p + 15) // 16 * 16


def rows_per_chunk(n, ncols, wide):
    """moments_device.hpp: dense_rows_per_chunk / wide_layout.hpp: wide_rows_per_chunk"""
    T = (ncols + TILE_COLS - 1) // TILE_COLS
    pairs = T * (T + 1) // 2
    if wide:
        cap = 1 if pairs >= 1024 else 1024 // pairs
        chunks = max(1, min((n + 255) // 256, cap))
    else:
        chunks = min(max(16, min(256, 1024 // pairs)), (n + 255) // 256)
    return -(-(-(-n // chunks)) // TILE_ROWS) * TILE_ROWS


def _gam(m):
    m = np.asarray(m, dtype=LD)
    return m * U / (1 - m * U)


def _gram(Da, Db, m):
    """Val of sum_i fl(Da_ia Db_ib): the products' roundings, then an any-order sum of m terms (m: a number or per entry)"""
    A, B = np.abs(Da.v), np.abs(Db.v)
    v, absum = Da.v.T @ Db.v, A.T @ B
    et = (A.T @ Db.e + Da.e.T @ B + Da.e.T @ Db.e) * (1 + U) + U * absum
    return Val(v, et + _gam(np.asarray(m) + 2) * (absum + et))


def _colsum(D, W, m):
    """Val of sum_i D_ia W_ib for exact 0/1 weights W (no product is formed): an any-order sum of m terms"""
    v = D.v.T @ W
    return Val(v, D.e.T @ W + _gam(np.asarray(m) + 2) * ((np.abs(D.v) + D.e).T @ W))


def _at(V, *idx):
    return Val(V.v[idx], V.e[idx])


def _where(c, a, b):
    return Val(np.where(c, a.v, b.v), np.where(c, a.e, b.e))


def _exact(a):
    return Val(np.asarray(a, dtype=LD))


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------

def _dense_and_stored(x):
    if sp.issparse(x):
        return N._dense_and_stored(x)
    xd = np.asarray(x, dtype=np.float64)
    return xd, np.ones(xd.shape, dtype=bool)


def make_case(name, x, y, *, fold=None, G=0, rest=False, centre=True, standardize=True, standardize_response=False, wide=False,
              scale=None, mixes=(0.0, 0.5), lam=(0.3, 0.1)):
    """y (n,): the one-response form; (n, K): the K-response form.  fold None: one fit (scale: what the driver would pass)."""
    xd, stored = _dense_and_stored(x)
    n, p = xd.shape
    y = np.asarray(y, dtype=np.float64)
    multi = y.ndim == 2
    Y = np.asfortranarray(y.reshape(n, -1))
    assert n <= 4096, "the reference's own rounding is covered up to 4096 terms"
    c = SimpleNamespace(name=name, x=x, xd=xd, stored=stored, sparse=sp.issparse(x), y=y, Y=Y, K=Y.shape[1], multi=multi, n=n, p=p,
                        fold=None if fold is None else np.asarray(fold, dtype=np.int32), G=int(G), rest=bool(rest), centre=bool(centre),
                        standardize=bool(standardize), standardize_response=bool(standardize_response), wide=bool(wide),
                        scale=scale, mixes=np.asarray(mixes, dtype=np.float64))
    c.lam = np.ascontiguousarray(np.broadcast_to(np.asarray(lam, dtype=np.float64), (len(mixes), len(lam))))
    return c


def _dense_x(rng, n, p):
    return rng.standard_normal((n, p)) * rng.uniform(0.5, 3.0, p) + rng.uniform(-1.0, 1.0, p)


def _responses(rng, x, K):
    n, p = x.shape
    xd = x.toarray() if sp.issparse(x) else x
    z = xd - xd.mean(axis=0)
    sd = z.std(axis=0)
    z = z / np.where(sd > 0, sd, 1.0)
    Y = z @ (rng.standard_normal((p, K)) * (rng.random((p, K)) < 0.5)) / np.sqrt(p) + rng.standard_normal((n, K)) + rng.uniform(-2, 2, K)
    return Y


def _y(rng, x, K, multi):
    Y = _responses(rng, x, max(K, 1))
    return Y if multi else Y[:, 0]


def labels(rng, n, G, kind, x=None):
    """random: every group non-empty, sizes unequal; sorted: cut along the sorted first column; sizes: given sizes, in row order"""
    if kind == "random":
        f = np.concatenate([np.arange(G), rng.integers(0, G, n - G)]) if n >= G else np.arange(n)
        return rng.permutation(f).astype(np.int32)
    if kind == "sorted":
        order = np.argsort(x[:, 0], kind="stable")
        f = np.empty(n, dtype=np.int32)
        f[order] = (np.arange(n) * G) // n
        return f
    sizes = kind
    assert sum(sizes) == n and len(sizes) == G
    return rng.permutation(np.repeat(np.arange(G), sizes)).astype(np.int32)


# dense cross-validations: name -> (n, p, K (0: the one-response form), G, labels, rest, centre, standardize, standardize_response)
# Pa = p + K + 1 on both sides of 16 and of 32 and at 33; n around the 64-row step, cov_sum's stride of 256 and one / two /
# more chunks; G in {1, 3, 10}; unequal groups, a group of one row, a group of exactly one chunk (256 rows at n = 1025), a group
# longer than a chunk; labels random and cut along a sorted column; train_on both ways; the three (centre, standardize).
CV_DENSE = {
    "n1": (1, 3, 0, 1, "random", False, True, True, False),
    "n63_Pa15": (63, 13, 0, 3, "random", True, True, True, False),
    "n64_Pa16": (64, 14, 0, 3, "sorted", False, True, False, False),
    "n65_Pa17": (65, 15, 0, 10, "random", True, False, False, False),
    "n256_Pa31": (256, 28, 2, 3, (1, 100, 155), True, True, True, True),
    "n257_Pa32_G1": (257, 29, 2, 1, "random", False, True, True, False),
    "n1025_Pa33": (1025, 29, 3, 3, (256, 600, 169), True, True, False, False),
    "K17": (65, 10, 17, 3, "random", False, True, True, False),
    "K257": (65, 2, 257, 3, "random", True, True, True, True),
    "limit_70x198": (70, COV_MAX_FEATURES, 0, 3, "random", False, True, True, False),
    "limit_K3": (70, mcov_max_features(3), 3, 3, "sorted", True, True, True, False),
    "mean1e6": (63, 13, 0, 3, "random", True, True, True, False),
}
MEAN_1E6_COLUMN = 4     # of the cases called mean1e6: mean 1e6, unit spread (raw X'X - n m m' loses ten digits there)
# wide: p in {199, 208, 209, 1025} (no pad at 208, a pad of 15 at 209 and 1025), n in {65, 257}
CV_WIDE = {
    "w65x199": (65, 199, 0, 3, "random", True, True, True, False),
    "w257x208": (257, 208, 0, 3, "sorted", False, True, False, False),
    "w65x209_K2": (65, 209, 2, 3, "random", True, True, True, True),
    "w257x209_K2": (257, 209, 2, 10, "random", False, False, False, False),
    "w65x1025": (65, 1025, 0, 3, "random", True, True, True, False),
}


def cv_dense_case(name, wide=None):
    table = CV_DENSE if name in CV_DENSE else CV_WIDE
    n, p, K, G, kind, rest, centre, std, stdr = table[name]
    rng = np.random.default_rng(abs(hash_name(name)))
    x = _dense_x(rng, n, p)
    y = _y(rng, x, K, K > 0)
    if name == "K17":
        y[:, 5] = 4.0                                  # a constant response
    if name == "mean1e6":
        x[:, MEAN_1E6_COLUMN] = 1e6 + rng.standard_normal(n)
    f = labels(rng, n, G, kind, x)
    return make_case(name, x, y, fold=f, G=G, rest=rest, centre=centre, standardize=std, standardize_response=stdr,
                     wide=(name in CV_WIDE) if wide is None else wide)


def hash_name(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) + 20250


def loo_case(wide=False):
    """G = n = 37, train_on = rest: the one-hot column whose only 1 is the held-out row of training set 5"""
    rng = np.random.default_rng(3737)
    x = _dense_x(rng, 37, 5)
    x[:, 2] = 0.0
    x[5, 2] = 1.0
    return make_case("loo37", x, _y(rng, x, 0, False), fold=np.arange(37), G=37, rest=True, wide=wide)


def degenerate_case(rest, multi, wide=False, standardize=True, standardize_response=True):
    """Columns constant on a training set but not on the data.  90 x 6, three groups of 30 rows in row order:
    column 1: an indicator that is 1 on some rows of group 0 only; column 3: integer-valued, 3 on groups 1 and 2 and varying on
    group 0; column 4: 7 on group 1 only.  train_on = fold: sets 1 and 2 see columns 1 and 3 constant, set 1 column 4 too;
    rest: set 0 (groups 1 and 2) sees columns 1 and 3 constant.  multi: response 1 is 2.5 off group 0 (constant on the same sets)."""
    rng = np.random.default_rng(9090 + rest + 2 * multi)
    n, f = 90, np.repeat(np.arange(3), 30).astype(np.int32)
    x = _dense_x(rng, n, 6)
    x[:, 1] = 0.0
    x[rng.choice(30, 11, replace=False), 1] = 1.0
    x[:, 3] = 3.0
    x[:30, 3] = rng.integers(-4, 9, 30)
    x[30:60, 4] = 7.0
    y = _y(rng, x, 3 if multi else 0, multi)
    if multi:
        y[30:, 1] = 2.5
    return make_case(f"degenerate_{'rest' if rest else 'fold'}_{'K3' if multi else 'K1'}", x, y, fold=f, G=3, rest=rest, wide=wide,
                     standardize=standardize, standardize_response=standardize_response and multi)


def constant_response_case(wide=False):
    """one response, constant on training set 1 (train_on = fold): sd_T(y) is 1, c~ and y~'y~ are exactly 0"""
    rng = np.random.default_rng(4141)
    x = _dense_x(rng, 60, 4)
    y = _y(rng, x, 0, False)
    f = np.repeat(np.arange(3), 20).astype(np.int32)
    y[20:40] = -1.75
    return make_case("constant_response", x, y, fold=f, G=3, rest=False, wide=wide)


def _grouped_sparse(n, centre, descending):
    """newton_reference.sparse_case's eleven columns and two more: one with no stored entry in group 1, one stored in group 2 only"""
    base = N.sparse_case(n, centre, descending)
    rng = np.random.default_rng(5000 + n)
    f = labels(rng, n, 3, "random")
    a = np.flatnonzero(f != 1)[::2]
    b = np.flatnonzero(f == 2)[::3]
    cols = [(a, rng.uniform(0.5, 2.0, len(a))), (b, rng.uniform(0.5, 2.0, len(b)))]
    xs = base.x.tocsc()
    indptr, indices, data = list(xs.indptr), [xs.indices], [xs.data]
    for r, v in cols:
        if descending:
            r, v = r[::-1], v[::-1]
        indices.append(r.astype(np.int32))
        data.append(v)
        indptr.append(indptr[-1] + len(r))
    x = sp.csc_matrix((np.concatenate(data), np.concatenate(indices).astype(np.int32), np.array(indptr, dtype=np.int32)),
                      shape=(n, xs.shape[1] + 2))
    return x, f, rng


# sparse cross-validations: name -> (n, K, G, rest, centre, standardize, descending)
CV_SPARSE = {
    "s600": (600, 0, 3, True, True, True, False),
    "s257_K2": (257, 2, 3, False, True, False, False),
    "s257_uncentred": (257, 0, 3, True, False, False, False),
    "s600_K3": (600, 3, 3, True, True, True, False),
}


def cv_sparse_case(name, descending=False, wide=False):
    n, K, G, rest, centre, std, _ = CV_SPARSE[name]
    x, f, rng = _grouped_sparse(n, centre, descending)
    return make_case(name + ("_desc" if descending else ""), x, _y(rng, x, K, K > 0), fold=f, G=G, rest=rest, centre=centre,
                     standardize=std, standardize_response=K > 0 and std, wide=wide)


def empty_sparse_cv_case(wide=False):
    rng = np.random.default_rng(66)
    return make_case("s_empty", sp.csc_matrix((50, 4)), rng.standard_normal(50), fold=labels(rng, 50, 3, "random"), G=3, rest=True, wide=wide)


# one fit, dense: name -> (n, p, K (0: the one-response form), wide)
SINGLE_DENSE = {
    "n1_P15": (1, 14, 0, False), "n63_P16": (63, 15, 0, False), "n64_P17": (64, 16, 0, False), "n65_P31": (65, 29, 2, False),
    "n256_P32": (256, 29, 3, False), "n257_P33_K17": (257, 16, 17, False), "n1025_P33": (1025, 32, 0, False),
    "K257": (65, 2, 257, False), "limit_70x198": (70, COV_MAX_FEATURES, 0, False), "limit_K3": (70, mcov_max_features(3), 3, False),
    "w65x199": (65, 199, 0, True), "w257x208": (257, 208, 0, True), "w65x209_K2": (65, 209, 2, True),
    "w257x209_K3": (257, 209, 3, True), "w65x1025": (65, 1025, 0, True), "mean1e6": (65, 15, 0, False),
}


def single_dense_case(name, centre=True):
    n, p, K, wide = SINGLE_DENSE[name]
    rng = np.random.default_rng(hash_name(name) + 7)
    x = _dense_x(rng, n, p)
    y = _y(rng, x, K, K > 0)
    y = y - y.mean(axis=0)                           # (as the driver hands it over: less the null model's intercepts)
    if name == "mean1e6":
        x[:, MEAN_1E6_COLUMN] = 1e6 + rng.standard_normal(n)
    return make_case(name, x, y, centre=centre, wide=wide, scale=rng.uniform(0.5, 2.0, p), mixes=(0.5,))


def single_sparse_case(n, K=0, descending=False, wide=False, centre=True):
    base = N.sparse_case(n, centre, descending)
    rng = np.random.default_rng(8100 + n)
    y = _y(rng, base.x, K, K > 0)
    return make_case(f"sparse{n}" + ("_desc" if descending else ""), base.x, y - y.mean(axis=0), centre=centre, wide=wide,
                     scale=base.scale, mixes=(0.5,))


def empty_sparse_single_case():
    rng = np.random.default_rng(67)
    return make_case("sparse_empty", sp.csc_matrix((50, 4)), rng.standard_normal(50), scale=np.ones(4), mixes=(0.5,))


# ---------------------------------------------------------------------------------------------------------------
# the stages in long double, with their bounds
# ---------------------------------------------------------------------------------------------------------------

def groups_of(case):
    """the row sets the moment matrices are taken over: the groups, or all rows (one fit)"""
    if case.fold is None:
        return [np.arange(case.n)]
    return [np.flatnonzero(case.fold == g) for g in range(case.G)]


def layout(case):
    """(grouped, nc = p + K, ncols of a moment matrix, index of the ones column or None)"""
    grouped = case.fold is not None
    nc = case.p + case.K
    return grouped, nc, nc + (1 if grouped else 0), (nc if grouped else None)


def mu_layout(case):
    """where the device keeps what: (length of mu, the K indices of the response sums, the K indices of their means or None)"""
    p, K = case.p, case.K
    if not case.multi:
        return p + 2, [p], [p + 1]
    if case.fold is None:
        return p + K, list(range(p, p + K)), None
    return p + 2 * K, list(range(p, p + K)), list(range(p + K, p + 2 * K))


def check_means(o, case):
    p, n = case.p, case.n
    size, sums, means = mu_layout(case)
    assert o.mu.shape == (size,), f"means: mu has shape {o.mu.shape}"
    if not case.centre:
        assert np.all(o.mu[:p] == 0.0) and not np.any(np.signbit(o.mu[:p])), "means: not exactly 0 without centring"
    N.inside(o.mu[:p], N.mean_reference(case.xd, case.stored, case.centre), f"{case.name}: means")
    N.inside(o.mu[sums], fl_sum(_exact(case.Y), np.ones(case.Y.shape, dtype=bool), 0), f"{case.name}: response sums")
    if means is not None:
        assert np.array_equal(o.mu[means], o.mu[sums] / float(n)), "response means: not the returned sum / n, bit for bit"


def deviations(case, mu, rows):
    """Val (rows x ncols) of the augmented rows about the returned centres, as the kernels form them"""
    grouped, nc, ncols, one = layout(case)
    _, _, means = mu_layout(case)
    p = case.p
    cen = np.asarray(mu[:p], dtype=LD)
    D = fl_sub(_exact(case.xd[rows]), _exact(np.broadcast_to(cen, (len(rows), p))))
    if grouped:
        Yd = fl_sub(_exact(case.Y[rows]), _exact(np.broadcast_to(np.asarray(mu[means], dtype=LD), (len(rows), case.K))))
    else:
        Yd = _exact(case.Y[rows])
    parts_v, parts_e = [D.v, Yd.v], [D.e, Yd.e]
    if grouped:
        parts_v.append(np.ones((len(rows), 1), dtype=LD))
        parts_e.append(np.zeros((len(rows), 1), dtype=LD))
    return Val(np.concatenate(parts_v, axis=1), np.concatenate(parts_e, axis=1))


def dense_moment_reference(case, mu):
    """per row set: Val (ncols x ncols)"""
    out = []
    for rows in groups_of(case):
        D = deviations(case, mu, rows)
        out.append(_gram(D, D, len(rows)))
    return out


def sparse_moment_reference(case, mu, M_returned):
    """per row set: the kernel's identity in long double with the returned n_g and response sums; (Val, defined mask)"""
    grouped, nc, ncols, one = layout(case)
    p, K, n = case.p, case.K, case.n
    m = np.asarray(mu[:p], dtype=LD)
    out = []
    for g, rows in enumerate(groups_of(case)):
        Mr = np.asarray(M_returned[g], dtype=np.float64)
        ng = LD(Mr[one, one]) if grouped else LD(n)
        S = case.stored[rows].astype(LD)
        D = deviations(case, mu, rows)
        Dx = Val(D.v[:, :p] * S, D.e[:, :p] * S)
        cnt = S.T @ S
        cj = np.diag(cnt)
        both = _gram(Dx, Dx, cnt)
        only = _colsum(Dx, 1 - S, cj[:, None] - cnt)            # only[j, k] = sum over J \ K of d_j
        nei = _exact(ng - (cj[:, None] + cj[None, :] - cnt))
        mj = _exact(np.broadcast_to(m[:, None], (p, p)))
        mk = _exact(np.broadcast_to(m[None, :], (p, p)))
        only_j, only_k = only, Val(only.v.T, only.e.T)
        C = fl_add(fl_sub(fl_sub(both, fl_mul(mk, only_j)), fl_mul(mj, only_k)), fl_mul(fl_mul(nei, mj), mk))
        Tv, Te = np.full((ncols, ncols), LD(np.nan)), np.full((ncols, ncols), LD(np.nan))
        defined = np.zeros((ncols, ncols), dtype=bool)
        Tv[:p, :p], Te[:p, :p] = C.v, C.e
        defined[:p, :p] = True
        # sum|terms| of the identity (for the printed ratios): what the kernel adds, not the centred products
        Ax, am = np.abs(Dx.v), np.abs(m)
        oa = Ax.T @ (1 - S)
        mag = np.zeros((ncols, ncols), dtype=LD)
        mag[:p, :p] = Ax.T @ Ax + am[None, :] * oa + am[:, None] * oa.T + nei.v * am[:, None] * am[None, :]
        # the response columns: a = sum_J fl(d_j y~), ys = sum_J y~, the bracket from the returned sum
        Yd = Val(D.v[:, p:nc], D.e[:, p:nc])
        a = _gram(Dx, Yd, cj[:, None])
        ys = Val(S.T @ Yd.v, S.T @ Yd.e + _gam(cj[:, None] + 2) * (S.T @ (np.abs(Yd.v) + Yd.e)))
        if grouped:
            sy = _exact(np.broadcast_to(np.asarray(Mr[p:nc, one], dtype=LD)[None, :], (p, K)))
            bracket = fl_sub(sy, ys)
        else:
            _, sums, _ = mu_layout(case)
            sy = _exact(np.broadcast_to(np.asarray(mu[sums], dtype=LD)[None, :], (p, K)))
            full = (cj == n)[:, None] & np.ones((1, K), dtype=bool)
            bracket = _where(full, _exact(np.zeros((p, K))), fl_sub(sy, ys))
        cy = fl_sub(a, fl_mul(_exact(np.broadcast_to(m[:, None], (p, K))), bracket))
        Tv[:p, p:nc], Te[:p, p:nc] = cy.v, cy.e
        mag[:p, p:nc] = Ax.T @ np.abs(Yd.v) + am[:, None] * (np.abs(sy.v) + S.T @ np.abs(Yd.v))
        mag[p:nc, :p] = mag[:p, p:nc].T
        Tv[p:nc, :p], Te[p:nc, :p] = cy.v.T, cy.e.T
        defined[:p, p:nc] = defined[p:nc, :p] = True
        if grouped:
            ones = np.ones((len(rows), 1), dtype=LD)
            sa = _colsum(Dx, ones, cj[:, None])
            c1 = fl_sub(sa, fl_mul(_exact((ng - cj)[:, None]), _exact(m[:, None])))
            Tv[:p, one], Te[:p, one] = c1.v[:, 0], c1.e[:, 0]
            Tv[one, :p], Te[one, :p] = c1.v[:, 0], c1.e[:, 0]
            # cov_group_response(s)_kernel: the response block, the sums and n_g
            Dy = Val(D.v[:, p:], D.e[:, p:])
            R = _gram(Dy, Dy, len(rows))
            sums = _colsum(Yd, ones, len(rows))
            Tv[p:, p:], Te[p:, p:] = R.v, R.e
            Tv[p:nc, one], Te[p:nc, one] = sums.v[:, 0], sums.e[:, 0]
            Tv[one, p:nc], Te[one, p:nc] = sums.v[:, 0], sums.e[:, 0]
            Tv[one, one], Te[one, one] = LD(len(rows)), 0
            defined[:, :] = True
            mag[:p, one] = mag[one, :p] = Ax.sum(axis=0) + (ng - cj) * am
            mag[p:, p:] = np.abs(Dy.v).T @ np.abs(Dy.v)
            # for the chain: the centred moments themselves.  The identity is exact algebra, so with the exact n_g (the corner
            # is checked bit for bit) and the exact response sums its value IS D'D; the returned response sums differ from the
            # exact ones by at most their own bound, which enters the response columns times |m_j|
            extra = np.zeros((ncols, ncols), dtype=LD)
            extra[:p, p:nc] = am[:, None] * Te[p:nc, one][None, :]
            extra[p:nc, :p] = extra[:p, p:nc].T
            chain = Val(D.v.T @ D.v, Te + extra)
        out.append((Val(Tv, Te), defined, mag, chain if grouped else None))
    return out


def check_moments(o, case, ratios=None):
    """Mg (a cross-validation) or M (one fit) against the reference formed from the returned mu"""
    grouped, nc, ncols, one = layout(case)
    Ms = o.Mg if grouped else o.M[None]
    assert Ms.shape == (len(groups_of(case)), ncols, ncols), f"moments: shape {Ms.shape}"
    refs = sparse_moment_reference(case, o.mu, Ms) if case.sparse else [(r, np.ones((ncols, ncols), dtype=bool), None, r) for r in dense_moment_reference(case, o.mu)]
    for g, ((ref, defined, mag, _), rows) in enumerate(zip(refs, groups_of(case))):
        M = Ms[g]
        sym = defined & defined.T
        assert np.array_equal(M[sym], M.T[sym]), f"{case.name}: moments symmetric: M[{g}] != M[{g}]' bit for bit"
        if grouped:
            assert M[one, one] == float(len(rows)), f"{case.name}: corner: M[{g}] has n_g = {M[one, one]}, the group has {len(rows)} rows"
        N.inside(M, ref, f"{case.name}: moments of row set {g}", mask=defined)
        if ratios is not None:
            Da = np.abs(deviations(case, o.mu, rows).v)
            scale = Da.T @ Da if mag is None else mag
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(defined & (scale > 0), ref.e / scale, 0)
            ratios["sparse moments" if case.sparse else "dense moments"] = max(ratios.get("sparse moments" if case.sparse else "dense moments", 0.0), float(r.max()))
    return [r[3] for r in refs]          # what the chain starts from: the centred moments and the bound of this stage


def check_total(o, case, ratios=None):
    if not case.rest:
        return
    ref = fl_sum(_exact(o.Mg), np.ones(o.Mg.shape, dtype=bool), 0)
    N.inside(o.total, ref, f"{case.name}: total")
    if ratios is not None:
        a = np.abs(o.Mg).sum(axis=0)
        ratios["total"] = max(ratios.get("total", 0.0), float(np.where(a > 0, ref.e / np.where(a > 0, a, 1), 0).max()))


def constant_rule(q, a_c, a_s, d, nT, n_summed):
    """DESIGN.md 4.5 in float64, operation for operation as covariance.hip: cov_constant_on_set has it: (constant, tol)"""
    with np.errstate(invalid="ignore", over="ignore"):
        tol = ((nT + n_summed) + 8.0) * EPS * ((a_c + (2.0 * np.abs(d)) * a_s) + (nT * d) * d)
        return ~(q > tol), tol


def set_moments_f64(Mg, total, t, rest):
    """(C, |total| + |group| magnitudes) of training set t in float64, as the kernels' C(j, k) forms them"""
    if rest:
        return total - Mg[t], np.abs(total) + np.abs(Mg[t])
    return Mg[t], np.abs(Mg[t])


def recentre_f64(C, s, d, nT, upper_order=True):
    """M^T in float64, the operands in the order of the smaller index first (wcov_recentred); symmetric bit for bit"""
    j, k = np.meshgrid(np.arange(len(s)), np.arange(len(s)), indexing="ij")
    lo, hi = (np.minimum(j, k), np.maximum(j, k)) if upper_order else (j, k)
    return ((C - d[lo] * s[hi]) - d[hi] * s[lo]) + (nT * d[lo]) * d[hi]


def constants_f64(Mg, total, t, case):
    """the rule on the returned moments: (constant flags of the p + K columns, q, tol), all float64"""
    grouped, nc, ncols, one = layout(case)
    C, A = set_moments_f64(Mg, total, t, case.rest)
    nT = C[one, one]
    with np.errstate(invalid="ignore", divide="ignore"):
        s = C[:nc, one]
        d = np.where((np.arange(nc) >= case.p) | case.centre, s / nT, 0.0)
        q = ((np.diag(C)[:nc] - d * s) - d * s) + (nT * d) * d
    const, tol = constant_rule(q, np.diag(A)[:nc], A[:nc, one], d, nT, case.G if case.rest else 0)
    return const, q, tol


def assemble_reference(MgV, totalV, mu, t, case, const, sd_given=None):
    """The assembly of training set t composed over Val inputs (exact ones: one stage in isolation; the moment stage's own
    reference: the whole chain).  const: the columns judged constant (scale 1, exact zeros).  Returns a namespace of Val:
    nT, s, d, rec (nc x nc, re-centred), var, sd (nc; 1 where constant or not scaled), mean (nc)."""
    grouped, nc, ncols, one = layout(case)
    p, K = case.p, case.K
    C = fl_sub(totalV, _at(MgV, t)) if case.rest else _at(MgV, t)
    nT = _at(C, one, one)
    s = _at(C, slice(0, nc), one)
    nTb = Val(np.broadcast_to(nT.v, (nc,)), np.broadcast_to(nT.e, (nc,)))
    centred = (np.arange(nc) >= p) | case.centre
    d = _where(centred, fl_div(s, nTb), _exact(np.zeros(nc)))
    row = lambda V: Val(np.broadcast_to(V.v[:, None], (nc, nc)), np.broadcast_to(V.e[:, None], (nc, nc)))
    col = lambda V: Val(np.broadcast_to(V.v[None, :], (nc, nc)), np.broadcast_to(V.e[None, :], (nc, nc)))
    nTm = Val(np.broadcast_to(nT.v, (nc, nc)), np.broadcast_to(nT.e, (nc, nc)))
    Cxx = _at(C, slice(0, nc), slice(0, nc))
    rec = fl_add(fl_sub(fl_sub(Cxx, fl_mul(row(d), col(s))), fl_mul(col(d), row(s))), fl_mul(fl_mul(nTm, row(d)), col(d)))
    q = _at(rec, np.arange(nc), np.arange(nc))
    var = fl_div(q, nTb)
    scaled = np.concatenate([np.full(p, case.standardize), np.full(K, case.standardize_response or not case.multi)]) & ~const
    safe = _where(scaled, var, _exact(np.ones(nc)))
    assert np.all(safe.v - safe.e > 0), f"{case.name}: a variance of set {t} is not bounded away from 0 although the rule lets it stand"
    sd = _where(scaled, fl_sqrt(safe), _exact(np.ones(nc)))
    cen = np.zeros(nc, dtype=LD)
    cen[:p] = np.asarray(mu[:p], dtype=LD)
    _, _, means = mu_layout(case)
    cen[p:] = np.asarray(mu[means], dtype=LD)
    mean = _where(centred, fl_add(_exact(cen), d), _exact(np.zeros(nc)))
    if case.multi and case.standardize_response:
        mean = _where(np.arange(nc) >= p, _exact(np.zeros(nc)), mean)
    return SimpleNamespace(nT=nT, s=s, d=d, rec=rec, q=q, var=var, sd=sd, mean=mean, const=const)


def path_inputs_reference(a, case):
    """what the path kernel reads, from an assembly `a`: narrow Mt (one response: (p + 1)^2; K: p x nc), yy, nulldev"""
    grouped, nc, ncols, one = layout(case)
    p, K = case.p, case.K
    sdy = Val(np.broadcast_to(a.sd.v[None, p:], (nc, K)), np.broadcast_to(a.sd.e[None, p:], (nc, K)))
    xy = fl_div(_at(a.rec, slice(0, nc), slice(p, nc)), sdy)                   # every row's response columns / sd_y
    Mt_v, Mt_e = a.rec.v.copy(), a.rec.e.copy()
    Mt_v[:, p:], Mt_e[:, p:] = xy.v, xy.e
    Mt = Val(Mt_v, Mt_e)
    if not case.multi:
        last = fl_div(_at(Mt, p, slice(0, nc)), Val(np.broadcast_to(a.sd.v[p], (nc,)), np.broadcast_to(a.sd.e[p], (nc,))))     # row p: / sd_y again
        Mt.v[p, :], Mt.e[p, :] = last.v, last.e
    zero = a.const[:, None] | a.const[None, :]
    Mt = _where(zero, _exact(np.zeros((nc, nc))), Mt)
    qy = _where(a.const[p:], _exact(np.zeros(K)), _at(a.q, slice(p, nc)))
    yy_terms = fl_div(fl_div(qy, _at(a.sd, slice(p, nc))), _at(a.sd, slice(p, nc)))
    yy = fl_sum(yy_terms, np.ones(K, dtype=bool), 0)
    nulldev = fl_sum(qy, np.ones(K, dtype=bool), 0)
    return SimpleNamespace(Mt=Mt, yy=yy, nulldev=nulldev)


def wide_reference(a, case, nT, f, ysd):
    """S_T (p x p), c~_T (p x K) from an assembly's re-centred matrix and the RETURNED n_T, scales f and response divisors"""
    p, K, nc = case.p, case.K, case.p + case.K
    nTm = _exact(np.full((p, p), LD(nT)))
    ff = fl_mul(_exact(np.broadcast_to(np.asarray(f, dtype=LD)[:, None], (p, p))), _exact(np.broadcast_to(np.asarray(f, dtype=LD)[None, :], (p, p))))
    S = fl_div(fl_div(_at(a.rec, slice(0, p), slice(0, p)), nTm), ff)
    ct = fl_div(fl_div(fl_div(_at(a.rec, slice(0, p), slice(p, nc)), _exact(np.broadcast_to(np.asarray(ysd, dtype=LD)[None, :], (p, K)))),
                       _exact(np.full((p, K), LD(nT)))), _exact(np.broadcast_to(np.asarray(f, dtype=LD)[:, None], (p, K))))
    cx = a.const[:p]
    S = _where(cx[:, None] | cx[None, :], _exact(np.zeros((p, p))), S)
    ct = _where(cx[:, None] | a.const[None, p:], _exact(np.zeros((p, K))), ct)
    return S, ct


def direct_truth(case, t):
    """the long-double moments of x[T], y[T] formed directly: n_T, means, M^T about them (nc x nc)"""
    rows = np.flatnonzero(case.fold != t) if case.rest else np.flatnonzero(case.fold == t)
    A = np.concatenate([case.xd[rows], case.Y[rows]], axis=1).astype(LD)
    mean = A.sum(axis=0) / len(rows)
    if not case.centre:
        mean[:case.p] = 0
    Z = A - mean
    return SimpleNamespace(rows=rows, nT=len(rows), mean=mean, M=Z.T @ Z)


def exactly_constant(case, t):
    """columns of [x | y] that are constant on training set t and exactly summable there (setup_reference.constant_columns)"""
    rows = np.flatnonzero(case.fold != t) if case.rest else np.flatnonzero(case.fold == t)
    A = np.concatenate([case.xd[rows], case.Y[rows]], axis=1)
    const = np.all(A == A[0], axis=0)
    if not case.centre:
        const[:case.p] &= A[0, :case.p] == 0            # about 0 an uncentred constant is a feature like any other
    for c in A[0, const]:
        assert len(rows) == 1 or (c == np.floor(4 * c) / 4 and abs(c) * len(rows) < 2.0 ** 50), "a constant that is not exactly summable"
    return const


MARGIN = 1e6     # measured: profiles/covariance_passes.txt has the smallest q / tol of a column that is not constant (1.8e12)


def constant_margin(o, case):
    """every exactly-constant column falls under the rule; no other comes within MARGIN of it.  Returns the smallest q / tol
    over the columns that are not constant (inf when there is none)."""
    smallest = np.inf
    for t in range(case.G):
        const, q, tol = constants_f64(o.Mg, o.total if case.rest else None, t, case)
        want = exactly_constant(case, t)
        assert np.all(const[want]), f"{case.name}: constant rule: set {t}, columns {np.flatnonzero(want & ~const)} are constant on T and above the rule"
        others = ~want
        if np.any(others):
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(tol[others] > 0, q[others] / tol[others], np.inf)
            assert np.all(r > MARGIN), f"{case.name}: constant rule: set {t}: a column that is not constant is within {r.min():.3g} of the rule"
            smallest = min(smallest, float(r.min()))
    return smallest


def product_moments_f64(case):
    """mu, Mg and total by float64 matrix products of the centred augmented rows (one more summation order; sparse x through
    its dense form): enough for constant_margin, which reads nothing else, at the cost of a BLAS call per group"""
    grouped, nc, ncols, one = layout(case)
    _, sums, means = mu_layout(case)
    mu = _mu_f64(case, seq_sum)
    A = np.concatenate([case.xd - mu[:case.p], case.Y - mu[means], np.ones((case.n, 1))], axis=1)
    o = SimpleNamespace(mu=mu, Mg=np.stack([A[rows].T @ A[rows] for rows in groups_of(case)]))
    o.Mg = 0.5 * (o.Mg + o.Mg.transpose(0, 2, 1))
    o.total = o.Mg.sum(axis=0)
    return o


def check_assembly(o, case, moment_refs=None, ratios=None):
    """every output of the assembly stage(s) of a cross-validation"""
    grouped, nc, ncols, one = layout(case)
    p, K, G = case.p, case.K, case.G
    A, L = len(case.mixes), case.lam.shape[1]
    name = case.name
    total = o.total if case.rest else None
    MgE, totE = _exact(o.Mg), (_exact(o.total) if case.rest else None)
    if moment_refs is not None:
        MgC = Val(np.stack([r.v for r in moment_refs]), np.stack([np.nan_to_num(r.e) for r in moment_refs]))
        totC = fl_sum(MgC, np.ones(MgC.v.shape, dtype=bool), 0) if case.rest else None
    assert o.ridge.shape == (A, G) and np.array_equal(o.ridge, np.broadcast_to((case.mixes == 0.0)[:, None], (A, G)).astype(float)), f"{name}: ridge"
    if case.wide:
        ld = wide_leading_dim(p)
        assert o.ld == ld and o.S.shape == (G, p, ld), f"{name}: ld: {o.ld}, S {o.S.shape}"
        assert np.all(o.S[:, :, p:] == 0.0) and not np.any(np.signbit(o.S[:, :, p:])), f"{name}: pad: rows p .. ld - 1 of S_T are not exactly 0"
        assert np.array_equal(o.S[:, :, :p], o.S[:, :, :p].transpose(0, 2, 1)), f"{name}: S_T symmetric: S_T[j, k] and S_T[k, j] differ in bits"
        assert np.array_equal(o.Sd, np.diagonal(o.S, axis1=1, axis2=2)), f"{name}: diag S_T: not the diagonal of S_T"
    for t in range(G):
        const, q64, tol = constants_f64(o.Mg, total, t, case)
        C64, _ = set_moments_f64(o.Mg, total, t, case.rest)
        a = assemble_reference(MgE, totE, o.mu, t, case, const)
        nT = C64[one, one]
        T = direct_truth(case, t)
        assert o.tstat[0, t] == nT == float(T.nT), f"{name}: n_T of set {t}: {o.tstat[0, t]}, the set has {T.nT} rows"
        cx, cy = const[:p], const[p:]
        if not case.standardize:
            assert np.all(o.scale[t] == 1.0), f"{name}: scale == 1 without standardize (set {t})"
        assert np.all(o.scale[t][cx] == 1.0), f"{name}: constant feature: scale of a column constant on set {t} is not exactly 1"
        N.inside(o.scale[t], _at(a.sd, slice(0, p)), f"{name}: scale of set {t}")
        if not case.centre:
            assert np.all(o.mean[t, :p] == 0.0), f"{name}: mean == 0 where not centred (set {t})"
        N.inside(o.mean[t], a.mean, f"{name}: mean of set {t}")
        pin = path_inputs_reference(a, case)
        if case.multi:
            N.inside(o.tstat[1, t], pin.yy, f"{name}: yy of set {t}")
            N.inside(o.tstat[2, t], pin.nulldev, f"{name}: nulldev of set {t}")
            if np.all(cy):
                assert o.tstat[1, t] == 0.0 and o.tstat[2, t] == 0.0, f"{name}: constant response: yy / nulldev of set {t} not exactly 0"
            l2 = (1.0 - case.mixes)[:, None] * case.lam
            l1 = case.mixes[:, None] * case.lam
            assert np.array_equal(o.pen_a[:, t], l2) and np.array_equal(o.pen_b[:, t], l1), f"{name}: penalties of set {t}"
            ysd = o.ysd[t] if case.wide else None
        else:
            sd_y = o.tstat[1, t]
            N.inside(sd_y, _at(a.sd, p), f"{name}: sd_y of set {t}")
            N.inside(o.tstat[2, t], pin.yy, f"{name}: yy of set {t}")
            if cy[0]:
                assert sd_y == 1.0 and o.tstat[2, t] == 0.0, f"{name}: constant response: sd_y / yy of set {t} not exactly 1 / 0"
            al = (1.0 - case.mixes)[:, None] * case.lam / sd_y
            be = case.mixes[:, None] * case.lam / sd_y
            assert np.array_equal(o.pen_a[:, t], al) and np.array_equal(o.pen_b[:, t], be), f"{name}: penalties of set {t}"
            ysd = np.array([sd_y])
        if case.wide:
            if case.multi:
                assert np.all(o.ysd[t][cy] == 1.0), f"{name}: constant response: ysd of set {t} not exactly 1"
                N.inside(o.ysd[t], _at(a.sd, slice(p, nc)), f"{name}: ysd of set {t}")
            # the stats kernel's s and d: one subtraction, one division
            with np.errstate(invalid="ignore", divide="ignore"):
                s64 = C64[:nc, one]
                d64 = np.where((np.arange(nc) >= p) | case.centre, s64 / nT, 0.0)
            assert np.array_equal(o.s[t], s64) and np.array_equal(o.d[t], d64), f"{name}: s, d of set {t}: not total - group and s / n_T bit for bit"
            # the assembly kernel from what the stats kernel RETURNED
            aw = SimpleNamespace(rec=_recentred_from(MgE, totE, t, case, o.s[t], o.d[t], nT), const=const)
            S, ct = wide_reference(aw, case, nT, o.scale[t], ysd)
            N.inside(o.S[t][:, :p], S, f"{name}: S_T of set {t}")
            N.inside(o.ct[t], ct, f"{name}: c~_T of set {t}")
            zero = cx[:, None] | cx[None, :]
            assert np.all(o.S[t][:, :p][zero] == 0.0) and np.all(o.ct[t][cx] == 0.0) and np.all(o.ct[t][:, cy] == 0.0), \
                f"{name}: constant column: row / column of S_T or c~_T of set {t} not exactly 0"
            got_S, got_c = o.S[t][:, :p], o.ct[t]
            f = o.scale[t]
        else:
            Mt = o.Mt[t]
            want = pin.Mt if not case.multi else _at(pin.Mt, slice(0, p), slice(0, nc))
            N.inside(Mt, want, f"{name}: Mt of set {t}")
            zero = (const[:, None] | const[None, :])[:Mt.shape[0]]
            assert np.all(Mt[zero] == 0.0), f"{name}: constant column: row / column of Mt of set {t} not exactly 0"
        if ratios is not None:
            mag = np.abs(C64[:nc, :nc]) + 2 * np.abs(np.outer(a.d.v, a.s.v)).astype(np.float64) + float(nT) * np.abs(np.outer(a.d.v, a.d.v)).astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(mag > 0, np.asarray(a.rec.e, dtype=np.float64) / mag, 0)
            ratios["assembly"] = max(ratios.get("assembly", 0.0), float(r.max()))
        # the whole chain against the moments of x[T], y[T] formed directly: the chain's own exact value IS those moments
        # (re-centring is exact algebra), so the device is held to the chain's bound about them (1 % for the long double's own rounding)
        if moment_refs is not None:
            ac = assemble_reference(MgC, totC, o.mu, t, case, const)
            live = ~(const[:, None] | const[None, :])
            assert np.all(np.abs(ac.rec.v - T.M)[live] <= 0.01 * ac.rec.e[live]), f"{name}: chain: the reference's own chain misses the direct moments (set {t})"
            chain = Val(T.M, 1.01 * ac.rec.e)
            if case.wide:
                Sc, cc = wide_reference(SimpleNamespace(rec=chain, const=const), case, nT, f, ysd)
                N.inside(got_S, Sc, f"{name}: chain: S_T of set {t} against the direct moments of x[T]", mask=live[:p, :p])
                N.inside(got_c, cc, f"{name}: chain: c~_T of set {t} against the direct moments", mask=live[:p, p:])
            else:
                exact_sd = np.where(ac.sd.v == 1, LD(1), np.sqrt(np.where(const, 1, np.diag(T.M) / T.nT)))
                exact_sd = np.where((ac.sd.v == 1) & (ac.sd.e == 0), LD(1), exact_sd)
                direct = path_inputs_reference(SimpleNamespace(rec=chain, q=_at(chain, np.arange(nc), np.arange(nc)),
                                                               sd=Val(exact_sd, 1.01 * ac.sd.e), const=const), case).Mt
                want = direct if not case.multi else _at(direct, slice(0, p), slice(0, nc))
                N.inside(o.Mt[t], want, f"{name}: chain: Mt of set {t} against the direct moments of x[T], y[T]", mask=live[:o.Mt[t].shape[0]])


def _recentred_from(MgE, totE, t, case, s, d, nT):
    """M^T (Val, nc x nc) from the returned moments and the RETURNED s, d, n_T (the wide assembly kernel's inputs)"""
    grouped, nc, ncols, one = layout(case)
    C = fl_sub(totE, _at(MgE, t)) if case.rest else _at(MgE, t)
    Cxx = _at(C, slice(0, nc), slice(0, nc))
    sv, dv = _exact(s), _exact(d)
    row = lambda V: Val(np.broadcast_to(V.v[:, None], (nc, nc)), np.zeros((nc, nc), dtype=LD))
    col = lambda V: Val(np.broadcast_to(V.v[None, :], (nc, nc)), np.zeros((nc, nc), dtype=LD))
    nTm = _exact(np.full((nc, nc), LD(nT)))
    return fl_add(fl_sub(fl_sub(Cxx, fl_mul(row(dv), col(sv))), fl_mul(col(dv), row(sv))), fl_mul(fl_mul(nTm, row(dv)), col(dv)))


def wide_from_narrow_f64(narrow, t, case):
    """S_T (j <= k) and c~_T restated in float64 from the NARROW assembly's returned Mt, scale and n_T: the expressions the
    code calls the same"""
    p, K = case.p, case.K
    f, nT = narrow.scale[t], narrow.tstat[0, t]
    Mt = narrow.Mt[t]
    S = Mt[:p, :p] / nT / (f[:, None] * f[None, :])
    ct = Mt[:p, p:p + K] / nT / f[:, None]
    return S, ct


def check_wide_equals_narrow(wide, narrow, case):
    for t in range(case.G):
        S, ct = wide_from_narrow_f64(narrow, t, case)
        iu = np.triu_indices(case.p)
        assert np.array_equal(wide.S[t][:, :case.p][iu], S[iu]), f"{case.name}: wide == narrow: S_T of set {t} differs from Mt / n_T / (f f') in bits"
        assert np.array_equal(wide.ct[t], ct), f"{case.name}: wide == narrow: c~_T of set {t} differs from Mt / n_T / f in bits"


def check_cv(o, case, ratios=None, chain=True):
    check_means(o, case)
    refs = check_moments(o, case, ratios)
    check_total(o, case, ratios)
    check_assembly(o, case, refs if chain else None, ratios)


def check_single(o, case, ratios=None):
    """one fit: means, M, and the scale stage bit for bit from the returned M"""
    p, K, n, nc = case.p, case.K, case.n, case.p + case.K
    check_means(o, case)
    check_moments(o, case, ratios)
    sc, M = case.scale, o.M
    c = M[:p, p:nc] / float(n) / sc[:, None]
    if case.wide:
        ld = wide_leading_dim(p)
        assert o.ld == ld and o.S.shape == (p, ld), f"{case.name}: ld: {o.ld}, S {o.S.shape}"
        assert np.all(o.S[:, p:] == 0.0) and not np.any(np.signbit(o.S[:, p:])), f"{case.name}: pad: rows p .. ld - 1 of S are not exactly 0"
        iu = np.triu_indices(p)
        S = np.zeros((p, p))
        S[iu] = (M[:p, :p] / float(n) / (sc[:, None] * sc[None, :]))[iu]
        S = np.where(np.arange(p)[:, None] <= np.arange(p)[None, :], S, S.T)
        assert np.array_equal(o.S[:, :p], S), f"{case.name}: scale: S is not M / n / (s s') from the upper triangle, bit for bit"
        assert np.array_equal(o.Sd, np.diag(S)), f"{case.name}: scale: diag S"
        assert np.array_equal(o.ct, c), f"{case.name}: scale: c~ is not M[j, p + r] / n / s_j, bit for bit"
    else:
        assert np.array_equal(o.c, c), f"{case.name}: scale: the path kernel's c is not M[j, p + r] / n / s_j, bit for bit"


def same_bits(a, b, what):
    for k, v in vars(a).items():
        w = getattr(b, k)
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, w, equal_nan=True), f"{what}: field {k} differs in bits"
        else:
            assert v == w, f"{what}: field {k}"


# ---------------------------------------------------------------------------------------------------------------
# float64 restatements of the kernels (fsum: one of newton_reference.SUMS) and the wrong versions the checks must reject
# ---------------------------------------------------------------------------------------------------------------

WRONG_MOMENTS = ("raw_moments", "no_in_neither", "union_miscounted", "other_groups_rows", "dropped_last_step", "chunk_to_neighbour",
                 "reduce_off_by_one", "total_missing_last")
WRONG_ASSEMBLY = ("d_not_zeroed", "sign_nTdd", "sdy_before_recentre", "n_for_nT", "c_not_div_sdy", "shift_neighbour",
                  "constant_response_kept", "nulldev_scaled", "nonzero_pad", "lower_unmirrored")
WRONG = WRONG_MOMENTS + WRONG_ASSEMBLY


def _mu_f64(case, fsum):
    size, sums, means = mu_layout(case)
    mu = np.zeros(size)
    mu[:case.p] = N.mean_f64(case.xd, case.stored, case.centre, fsum)
    mu[sums] = [fsum(case.Y[:, r]) for r in range(case.K)]
    if means is not None:
        mu[means] = mu[sums] / float(case.n)
    return mu


def _terms_sum(A, B, fsum):
    """sum_i A_ia B_ib by fsum, in column blocks to bound the memory"""
    out = np.empty((A.shape[1], B.shape[1]))
    step = max(1, (1 << 22) // max(1, A.shape[0] * B.shape[1]))
    for a0 in range(0, A.shape[1], step):
        out[a0:a0 + step] = fsum(A[:, a0:a0 + step, None] * B[:, None, :]) if A.shape[0] else 0.0
    return out


def dense_moments_f64(case, mu, fsum, wrong=None):
    grouped, nc, ncols, one = layout(case)
    _, _, means = mu_layout(case)
    p = case.p
    A = np.concatenate([case.xd - mu[:p], case.Y - mu[means] if grouped else case.Y] + ([np.ones((case.n, 1))] if grouped else []), axis=1)
    rpc = rows_per_chunk(case.n, ncols, case.wide)
    groups = groups_of(case)
    chunks, owner = [], []
    for g, rows in enumerate(groups):
        for r0 in range(0, len(rows), rpc):
            rr = rows[r0:r0 + rpc]
            if wrong == "dropped_last_step":
                rr = rr[:len(rr) // TILE_ROWS * TILE_ROWS]
            chunks.append(rr)
            owner.append(g)
    owner = np.array(owner)
    if wrong == "chunk_to_neighbour" and len(groups) > 1:
        last = [np.flatnonzero(owner == g)[-1] for g in range(len(groups) - 1)]
        owner[last] += 1
    part = [_terms_sum(A[rr], A[rr], fsum) for rr in chunks]
    Ms = []
    for g in range(len(groups)):
        mine = [part[c] for c in np.flatnonzero(owner == g)]
        if wrong == "reduce_off_by_one":
            mine = mine[:-1]
        Ms.append(seq_sum(np.stack(mine)) if mine else np.zeros((ncols, ncols)))
    Ms = np.stack(Ms)
    if wrong == "raw_moments":
        raw = np.concatenate([case.xd, A[:, p:]], axis=1)
        for g, rows in enumerate(groups):
            m = np.concatenate([mu[:p], np.zeros(ncols - p)])
            R = _terms_sum(raw[rows], raw[rows], fsum)
            sm = fsum(raw[rows])
            W = R - np.outer(m, sm) - np.outer(sm, m) + len(rows) * np.outer(m, m)
            Ms[g] = np.triu(W) + np.triu(W, 1).T
    return Ms


def sparse_moments_f64(case, mu, fsum, wrong=None):
    grouped, nc, ncols, one = layout(case)
    _, sums, means = mu_layout(case)
    p, K, n = case.p, case.K, case.n
    Ms = []
    for g, rows in enumerate(groups_of(case)):
        M = np.full((ncols, ncols), np.nan)
        Yd = case.Y[rows] - mu[means] if grouped else case.Y[rows]
        ng = float(len(rows))
        if grouped:
            for r in range(K):
                for t in range(r, K):
                    M[p + r, p + t] = M[p + t, p + r] = fsum(Yd[:, r] * Yd[:, t])
                M[p + r, one] = M[one, p + r] = fsum(Yd[:, r])
            M[one, one] = ng
        S = case.stored[rows]
        D = case.xd[rows] - mu[:p]
        for j in range(p):
            J = S[:, j]
            for k in range(j, p):
                Kk = S[:, k]
                if wrong == "other_groups_rows" and grouped:
                    both = fsum(((case.xd[:, j] - mu[j]) * (case.xd[:, k] - mu[k]))[case.stored[:, j] & case.stored[:, k]])
                else:
                    both = fsum((D[:, j] * D[:, k])[J & Kk])
                only_j, only_k = fsum(D[J & ~Kk, j]), fsum(D[Kk & ~J, k])
                cnt = float((J & Kk).sum())
                union = float(J.sum()) + float(Kk.sum()) - (0.0 if wrong == "union_miscounted" else cnt)
                nei = 0.0 if wrong == "no_in_neither" else ng - union
                M[j, k] = M[k, j] = both - mu[k] * only_j - mu[j] * only_k + nei * mu[j] * mu[k]
            for r in range(K):
                a, ys = fsum(D[J, j] * Yd[J, r]), fsum(Yd[J, r])
                rest = (M[p + r, one] - ys) if grouped else (0.0 if J.sum() == n else mu[sums[r]] - ys)
                M[j, p + r] = M[p + r, j] = a - mu[j] * rest
            if grouped:
                M[j, one] = M[one, j] = fsum(D[J, j]) - (ng - float(J.sum())) * mu[j]
        Ms.append(M)
    return np.stack(Ms)


def restate_single(case, fsum=seq_sum, wrong=None):
    p, K, n, nc = case.p, case.K, case.n, case.p + case.K
    o = SimpleNamespace(mu=_mu_f64(case, fsum))
    o.M = (sparse_moments_f64 if case.sparse else dense_moments_f64)(case, o.mu, fsum, wrong)[0]
    c = o.M[:p, p:nc] / float(n) / case.scale[:, None]
    if case.wide:
        o.ld = wide_leading_dim(p)
        S = o.M[:p, :p] / float(n) / (case.scale[:, None] * case.scale[None, :])
        o.S = np.zeros((p, o.ld))
        o.S[:, :p] = np.where(np.arange(p)[:, None] <= np.arange(p)[None, :], S, S.T)
        if wrong == "nonzero_pad" and o.ld > p:
            o.S[:, p:] = 1e-300
        o.Sd, o.ct = np.diag(o.S[:, :p]).copy(), c
    else:
        o.c = c
    return o


def restate_cv(case, fsum=seq_sum, wrong=None, given=None):
    """covariance_cv_run / mcovariance_cv_run / wcovariance_cv_run / wmcovariance_cv_run up to the path kernel, in float64.
    given: a result whose mu, Mg and total are taken as they are (the assembly alone is restated)"""
    grouped, nc, ncols, one = layout(case)
    p, K, G = case.p, case.K, case.G
    A, L = len(case.mixes), case.lam.shape[1]
    _, _, means = mu_layout(case)
    if given is not None:
        o = SimpleNamespace(mu=given.mu, Mg=given.Mg)
        if case.rest:
            o.total = given.total
    else:
        o = SimpleNamespace(mu=_mu_f64(case, fsum))
        o.Mg = (sparse_moments_f64 if case.sparse else dense_moments_f64)(case, o.mu, fsum, wrong)
        if case.rest:
            o.total = fsum(o.Mg[:-1] if wrong == "total_missing_last" else o.Mg)
    o.scale, o.mean, o.tstat = np.ones((G, p)), np.zeros((G, nc)), np.zeros((3, G))
    o.pen_a, o.pen_b, o.ridge = np.zeros((A, G, L)), np.zeros((A, G, L)), np.zeros((A, G))
    if case.wide:
        o.ld = wide_leading_dim(p)
        o.s, o.d, o.S, o.Sd, o.ct = np.zeros((G, nc)), np.zeros((G, nc)), np.zeros((G, p, o.ld)), np.zeros((G, p)), np.zeros((G, p, K))
        if case.multi:
            o.ysd = np.ones((G, K))
    else:
        o.Mt = np.zeros((G, p, nc) if case.multi else (G, p + 1, p + 1))
    scaled_y = case.standardize_response or not case.multi
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(G):
            C, Amag = set_moments_f64(o.Mg, o.total if case.rest else None, t, case.rest)
            nT = C[one, one]
            s = C[:nc, one].copy()
            centred = (np.arange(nc) >= p) | case.centre | (wrong == "d_not_zeroed")
            d = np.where(centred, s / nT, 0.0)
            if wrong == "shift_neighbour" and K > 1:
                d[p:] = np.roll(d[p:], 1)
            rec = recentre_f64(C[:nc, :nc], s, d, nT, upper_order=wrong != "lower_unmirrored")
            if wrong == "sign_nTdd":
                rec = ((C[:nc, :nc] - np.outer(d, s)) - np.outer(s, d)) - (nT * d)[:, None] * d[None, :]
            q = np.diag(rec).copy()
            const, _ = constant_rule(q, np.diag(Amag)[:nc], Amag[:nc, one], d, nT, G if case.rest else 0)
            if wrong == "constant_response_kept":
                const[p:] = False
            var = q / (float(case.n) if wrong == "n_for_nT" else nT)
            if wrong == "sdy_before_recentre":
                var[p:] = np.diag(C)[p:nc] / nT
            sd = np.ones(nc)
            sd[:p] = np.where(case.standardize & ~const[:p], np.sqrt(np.where(const[:p], 1.0, var[:p])), 1.0)
            if wrong == "constant_response_kept":
                sd[p:] = np.sqrt(np.maximum(var[p:], 0.0)) if scaled_y else 1.0
            else:
                sd[p:] = np.where(scaled_y & ~const[p:], np.sqrt(np.where(const[p:], 1.0, var[p:])), 1.0)
            o.scale[t] = sd[:p]
            o.mean[t, :p] = np.where(case.centre, o.mu[:p] + d[:p], 0.0)
            o.mean[t, p:] = 0.0 if (case.multi and case.standardize_response) else o.mu[means] + d[p:]
            qy = np.where(const[p:], 0.0, q[p:])
            if case.multi:
                yy = nd = 0.0
                for r in range(K):
                    nd += qy[r] / sd[p + r] / sd[p + r] if wrong == "nulldev_scaled" else qy[r]
                    yy += qy[r] / sd[p + r] / sd[p + r]
                o.tstat[:, t] = nT, yy, nd
                o.pen_a[:, t], o.pen_b[:, t] = (1.0 - case.mixes)[:, None] * case.lam, case.mixes[:, None] * case.lam
            else:
                o.tstat[:, t] = nT, sd[p], qy[0] / sd[p] / sd[p]
                o.pen_a[:, t], o.pen_b[:, t] = (1.0 - case.mixes)[:, None] * case.lam / sd[p], case.mixes[:, None] * case.lam / sd[p]
            o.ridge[:, t] = case.mixes == 0.0
            zero = const[:, None] | const[None, :]
            ysd = np.ones(K) if wrong == "c_not_div_sdy" else sd[p:]
            if case.wide:
                o.s[t], o.d[t] = s, d
                if case.multi:
                    o.ysd[t] = sd[p:]
                f = sd[:p]
                S = np.where(zero[:p, :p], 0.0, rec[:p, :p] / nT / (f[:, None] * f[None, :]))
                o.S[t, :, :p] = S
                if wrong == "nonzero_pad" and o.ld > p:
                    o.S[t, :, p:] = 1e-300
                o.Sd[t] = np.diag(S)
                o.ct[t] = np.where(zero[:p, p:], 0.0, rec[:p, p:] / ysd[None, :] / nT / f[:, None])
            else:
                Mt = rec.copy()
                Mt[:, p:] = Mt[:, p:] / ysd[None, :]
                if not case.multi:
                    Mt[p, :] = Mt[p, :] / (1.0 if wrong == "c_not_div_sdy" else sd[p])
                Mt = np.where(zero, 0.0, Mt)
                o.Mt[t] = Mt[:p] if case.multi else Mt
    return o
