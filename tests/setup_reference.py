"""Pure-numpy reference of the device setup passes (sgdnet_amd/csrc/setup_device.hip), shared by
tests/test_setup_reference.py (CPU) and tests/test_gpu_setup_passes.py (GPU): exact (np.longdouble) column moments,
x'y and row norms from the dense form of the input, rounding-error bounds composed step by step over the kernels'
arithmetic, the record geometry restated from the row-length histogram, a decoder of the packed records, the
eigenvalues behind L_F, and the inputs both test modules use.

Error model.  u = 2^-53.  Every double operation rounds once: fl(a op b) = (a op b)(1 + d), |d| <= u (the library is
built without contraction; a fused multiply-add would round once instead of twice and stay inside the same bound).
A double sum of m terms IN ANY ORDER errs by at most gamma_m * sum|t_i|, gamma_m = m u / (1 - m u) (Higham,
Accuracy and Stability of Numerical Algorithms, 4.2).  `Val` carries the exact value v of a quantity and a bound e on
|computed - v|; the fl_* functions below propagate (v, e) through one operation each:
    sub / add   e = ea + eb,                       then + u (|v| + e) for the rounding
    mul         e = |a| eb + |b| ea + ea eb,       then + u (|v| + e)
    div         e = (ea + |a / b| eb) / (|b| - eb), then + u (|v| + e)      (from |a^/b^ - a/b| = |(a^-a) b - a (b^-b)| / |b^ b|)
    sqrt        e = ea / sqrt(a)  (|sqrt a^ - sqrt a| = |a^ - a| / (sqrt a^ + sqrt a) <= ea / sqrt a), then + 2 u (|v| + e):
                HIP documents sqrt(double) to 1 ulp = 2 u, not to half an ulp
    sum of m    e = sum e_i + gamma_(m+2) * sum (|t_i| + e_i)
The two extra terms in gamma_(m+2) pay for the reference itself: it is summed in 80-bit long double (unit roundoff
2^-64), which over m <= 4096 terms errs by at most m 2^-64 <= 2 u relative to sum|t_i| (asserted below).
Nothing in here was fitted to what a device returns."""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

LD = np.longdouble
U = LD(2.0) ** -53
OVF_STRIDE, OVF_CAP = 256, 20


def gamma(m):
    m = LD(m)
    return m * U / (1 - m * U)


class Val:
    """exact value v (long double) and a bound e on |computed - v|"""

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=LD)
        self.e = np.zeros_like(self.v) if e is None else np.broadcast_to(np.asarray(e, dtype=LD), self.v.shape).copy()


def _rounded(v, e, ulps=1):
    return Val(v, e + ulps * U * (np.abs(v) + e))


def fl_sub(a, b):
    return _rounded(a.v - b.v, a.e + b.e)


def fl_add(a, b):
    return _rounded(a.v + b.v, a.e + b.e)


def fl_mul(a, b):
    return _rounded(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e)


def fl_div(a, b):
    den = np.abs(b.v) - b.e
    assert np.all(den > 0), "divisor not bounded away from zero"
    v = a.v / b.v
    return _rounded(v, (a.e + np.abs(v) * b.e) / den)


def fl_sqrt(a):
    v = np.sqrt(a.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(a.v > 0, a.e / np.where(v > 0, v, 1), np.sqrt(a.e))   # v = 0: sqrt(a^) <= sqrt(ea)
    return _rounded(v, e, ulps=2)


def fl_sum(t, mask, axis):
    """sum over `axis` of the terms where mask holds, in any order; m = the largest number of terms of one sum"""
    assert t.v.shape[axis] <= 4096, "the reference's own rounding is covered up to 4096 terms"
    m = int(mask.sum(axis=axis).max()) if mask.size else 0
    tv, te = np.where(mask, t.v, 0), np.where(mask, t.e, 0)
    return Val(tv.sum(axis=axis), te.sum(axis=axis) + gamma(m + 2) * (np.abs(tv) + te).sum(axis=axis))


assert np.finfo(LD).eps <= 2.0 ** -63, "the reference needs an 80-bit (or wider) long double"


# ---------------------------------------------------------------------------------------------------------------
# exact moments
# ---------------------------------------------------------------------------------------------------------------

def dense_of(x):
    return np.asarray(x.toarray() if sp.issparse(x) else x, dtype=np.float64)


def exact_moments(x, ymap, standardize, sparse):
    """Long-double truth from the dense form of x.  sparse: the sparse passes scale the stored values and centre
    implicitly (mean_sq and x'y are those of x / sd); the dense passes centre and scale (those of (x - mean) / sd).
    The row norm is the centred one either way, from the centred matrix itself."""
    X = dense_of(x).astype(LD)
    n, p = X.shape
    Y = np.asarray(ymap, dtype=LD).reshape(n, -1)
    mean = X.sum(axis=0) / n
    var = ((X - mean) ** 2).sum(axis=0) / n
    sd = np.where(var == 0, LD(1), np.sqrt(var))
    if not standardize:
        mean, sd = np.zeros(p, dtype=LD), np.ones(p, dtype=LD)
    Z = (X - mean) / sd                      # what the solvers see
    P = X / sd if sparse else Z              # what the passes hold explicitly
    return SimpleNamespace(mean=mean, sd=sd, var=var, mean_sq=(P ** 2).sum(axis=0) / n, xty=P.T @ Y,
                           row_sqnorm=(Z ** 2).sum(axis=1), max_sqnorm=(Z ** 2).sum(axis=1).max())


def constant_columns(x):
    """columns whose population variance is exactly 0 (empty or constant); asserts that the kernels see that too:
    every partial sum of such a column is exact (n = 1, zeros, or an integer constant with n |c| < 2^53), so the mean
    is the constant, every deviation is 0 and the sd is exactly 1.  Inexact constants (0.1, say) are left out: their
    float sum depends on the order, in the reference as much as in the kernel."""
    X = dense_of(x)
    n = X.shape[0]
    const = np.all(X == X[0], axis=0)
    for c in X[0, const]:
        assert n == 1 or (c == np.floor(c) and abs(c) * n < 2.0 ** 53), "constant column that is not exactly summable"
    return const


def moment_bounds(x, ymap, standardize, sparse):
    """Bounds on |device - exact| for center, scale, mean_sq (per column), xty (p x cols) and max_sqnorm, composed over
    the arithmetic of col_stats_kernel / xt_times_kernel / row_norm_kernel (sparse) or dense_col_stats_kernel /
    dense_xt_times_kernel / dense_row_norm_kernel (dense), with every sum in any order:

      mean      s = sum x (k stored terms; dense: n), mean = s / n
      sd        sparse: var = sum_stored ((x - mean)^2 / n)  +  (n - k) * mean * mean / n;   dense: var = (sum (x - mean)^2) / n
                sd = sqrt(var); a column of variance exactly 0 (constant_columns) gives exactly 1: bound 0
      mean_sq   sparse: xs = x / sd, mean_sq = (sum xs^2) / n;   dense: z = (x - mean) / sd, mean_sq = (sum z^2) / n
      x'y       sum xs * y   (dense: z * y), y exact
      row norm  dense: sum_j z^2;   sparse, not standardised: sum_stored x^2;
                sparse, standardised: c = mean / sd, sum_stored (xs - c)^2 + (csq - cnz) with csq = sum_j c^2 over all p
                features and cnz = sum_stored c^2 -- the identity cancels, so the error is of the size of csq, not of the
                norm: that is what the composition gives, term by term.
                |max a - max b| <= max |a - b|: the bound on the maximum is the largest row bound.
    Precondition (asserted): |mean| <= 10 sd on every non-constant column, so that the sd is well conditioned."""
    X = dense_of(x).astype(LD)
    n, p = X.shape
    Y = np.asarray(ymap, dtype=LD).reshape(n, -1)
    stored = (X != 0) if sparse else np.ones(X.shape, dtype=bool)
    ex = exact_moments(x, ymap, standardize, sparse)
    const = constant_columns(x)
    nn = Val(LD(n))
    xv = Val(X)
    if standardize:
        assert np.all(np.abs(ex.mean[~const]) <= 10 * ex.sd[~const]), "|mean| <= 10 sd is the bound's precondition"
        mean = fl_div(fl_sum(xv, stored, 0), nn)
        mean.e[const] = 0
        dlt = fl_sub(xv, Val(mean.v[None, :], mean.e[None, :]))
        if sparse:
            var = fl_sum(fl_div(fl_mul(dlt, dlt), nn), stored, 0)
            k = Val(stored.sum(axis=0).astype(LD))
            var = fl_add(var, fl_div(fl_mul(fl_mul(fl_sub(nn, k), mean), mean), nn))
        else:
            var = fl_div(fl_sum(fl_mul(dlt, dlt), stored, 0), nn)
        # a constant column: var = 0 exactly -> sd = 1 exactly; keep the chain below well defined for it
        var_nc = Val(np.where(const, 1, var.v), np.where(const, 0, var.e))
        sd = fl_sqrt(var_nc)
        sd = Val(np.where(const, 1, sd.v), np.where(const, 0, sd.e))
        assert np.allclose(np.asarray(sd.v, dtype=np.float64), np.asarray(ex.sd, dtype=np.float64), rtol=1e-12)
    else:
        mean, sd = Val(np.zeros(p, dtype=LD)), Val(np.ones(p, dtype=LD))
        dlt = xv
    sdr = Val(sd.v[None, :], sd.e[None, :])
    if standardize:
        held = fl_div(xv if sparse else dlt, sdr)          # the values the passes hold: x / sd, or (x - mean) / sd
    else:
        held = xv                                          # untouched
    msq = fl_div(fl_sum(fl_mul(held, held), stored, 0), nn)
    xty_e = np.stack([fl_sum(fl_mul(held, Val(Y[:, c:c + 1] + 0 * X)), stored, 0).e for c in range(Y.shape[1])], axis=1)
    if sparse and standardize:
        c = fl_div(mean, sd)
        cc = fl_mul(c, c)
        csq = fl_sum(cc, np.ones(p, dtype=bool), 0)
        ccr = Val(np.broadcast_to(cc.v, X.shape), np.broadcast_to(cc.e, X.shape))
        cnz = fl_sum(ccr, stored, 1)
        d = fl_sub(held, Val(np.broadcast_to(c.v, X.shape), np.broadcast_to(c.e, X.shape)))
        rows = fl_add(fl_sum(fl_mul(d, d), stored, 1), fl_sub(Val(np.broadcast_to(csq.v, (n,)), np.broadcast_to(csq.e, (n,))), cnz))
    else:
        rows = fl_sum(fl_mul(held, held), stored, 1)
    assert np.allclose(np.asarray(rows.v, dtype=np.float64), np.asarray(ex.row_sqnorm, dtype=np.float64), rtol=1e-9, atol=1e-12)
    return SimpleNamespace(center=mean.e, scale=sd.e, mean_sq=msq.e, xty=xty_e, max_sqnorm=rows.e.max(), exact=ex)


def lambda_max_bound(x, y, family, standardize, lam0):
    """Bound on |lambda_[0] * max(alpha, 0.001) - kkt_reference.lambda_max| for sparse x on the device path.
    lambda_max = max_j |sum_i xs_ij yc_ik| / n (mgaussian: the 2-norm over k), xs = x / sd, yc = the centred response
    (class indicators for multinomial).  The driver divides yc by the response's sd before the product and multiplies
    the sd back afterwards.  Per (j, k):
      the x'y bound of moment_bounds for ymap = yc                                  (the kernel's sum, the device's sd)
      + sum_i |xs_ij| * gamma_(n+2) mean|y_k|       the float64 mean of y that yc is taken from (x is not centred, so a
                                                    constant shift of yc does not cancel)
      + 8 u sum_i |xs_ij yc_ik|                     yc = (y - ybar) / ysd (mgaussian: standardised twice), * ysd * y_scale:
                                                    at most eight roundings beside the product's own
    all divided by n; |norm a - norm b| <= norm(a - b) over k and |max a - max b| <= max |a - b| over j.  The whole is
    taken twice: the reference is a float64 numpy product that makes errors of the same kind.  lambda_[0] itself is
    exp(log(lambda_max / mix)): (|log lambda_0| + 4) * 2 u relative on top."""
    X = dense_of(x).astype(LD)
    n = X.shape[0]
    y = np.asarray(y, dtype=np.float64)
    Y = (y.reshape(-1, 1) == np.arange(int(y.max()) + 1)).astype(np.float64) if family == "multinomial" else y.reshape(n, -1)
    Yl = Y.astype(LD)
    Yc = Yl - Yl.sum(axis=0) / n
    B = moment_bounds(x, np.asarray(Yc, dtype=np.float64), standardize, True)
    held = np.abs(X / B.exact.sd)
    e = B.xty + held.sum(axis=0)[:, None] * (gamma(n + 2) * np.abs(Yl).mean(axis=0))[None, :] + 8 * U * (held.T @ np.abs(Yc))
    # (the float64 rounding of Yc handed to moment_bounds: one more u per term, inside the 8 u: the
    # binomial / gaussian / multinomial chains use five)
    per_feature = np.sqrt((e ** 2).sum(axis=1)) if family == "mgaussian" else e.max(axis=1)
    return float(2 * per_feature.max() / n + (abs(np.log(lam0)) + 4) * 2 * U * lam0)


# ---------------------------------------------------------------------------------------------------------------
# sample-major form, record geometry, record decoder
# ---------------------------------------------------------------------------------------------------------------

def sample_major(x):
    """(sptr, sidx, pos): scipy's CSR of x with sorted indices; pos[i] = the position in the CSC data of CSR entry i"""
    csc = x.tocsc()
    tag = sp.csc_matrix((np.arange(1, csc.nnz + 1, dtype=np.float64), csc.indices, csc.indptr), shape=csc.shape)
    csr = tag.tocsr()
    csr.sort_indices()
    return csr.indptr.astype(np.int64), csr.indices.astype(np.int32), (csr.data - 1).astype(np.int64)


def rec_bytes(c):
    return 16 + ((4 * c + 7) & ~7) + 8 * c


def record_geometry(row_nnz, rec_align):
    """batched_device.hpp / device_setup_finish: the cap is the row length the 90th percentile row has (at least 1);
    when that is 64 or more the histogram has no resolution left and the cap is the longest row, at most 512; the stride
    is the record of that cap rounded up to rec_align, and the cap grows into the slack.  Rows longer than the cap go on
    in overflow records of 20 entries."""
    z = np.asarray(row_nnz, dtype=np.int64)
    n = len(z)
    hist = np.bincount(np.minimum(z, 64), minlength=65)
    want = int(0.9 * float(n))
    acc, cap = 0, 1
    for b in range(65):
        acc += int(hist[b])
        cap = max(b, 1)
        if acc >= want:
            break
    if cap >= 64:
        cap = int(min(z.max(), 512))
    stride = -(-rec_bytes(cap) // rec_align) * rec_align
    while rec_bytes(cap + 1) <= stride:
        cap += 1
    blocks = np.where(z > cap, -(-(z - cap) // OVF_CAP), 0)
    return SimpleNamespace(stride=stride, cap=cap, val_off=16 + ((4 * cap + 7) & ~7), blocks=blocks, n_ovf=int(blocks.sum()))


def decode_records(rec, ovf, n, stride, cap, val_off):
    """The raw bytes back into rows.  Per row: y, nnz, first (the id of its first overflow record), idx[cap] and val[cap]
    of the main record INCLUDING the padding lanes, and chain: [(id, next, cnt, idx[20], val[20])] of its overflow
    records, followed by next-ids for as long as entries remain.  Bytes no field covers (the pad between idx and val, the
    slack behind val, the last 8 bytes of an overflow record) are not read: nothing defines them."""
    rec = np.ascontiguousarray(rec, dtype=np.uint8)
    ovf = np.ascontiguousarray(ovf, dtype=np.uint8)
    n_ovf = len(ovf) // OVF_STRIDE
    rows = []
    for i in range(n):
        b = rec[i * stride:(i + 1) * stride]
        y = b[0:8].view(np.float64)[0]
        nnz, first = (int(v) for v in b[8:16].view(np.int32))
        idx = b[16:16 + 4 * cap].view(np.int32).copy()
        val = b[val_off:val_off + 8 * cap].view(np.float64).copy()
        chain, rem, oid = [], nnz - min(nnz, cap), first
        while rem > 0:
            assert 0 <= oid < n_ovf, f"row {i}: overflow id {oid} outside the {n_ovf} records"
            o = ovf[oid * OVF_STRIDE:(oid + 1) * OVF_STRIDE]
            nxt, cnt = (int(v) for v in o[0:8].view(np.int32))
            assert 1 <= cnt <= OVF_CAP, f"row {i}: overflow record {oid} holds {cnt} entries"
            chain.append((oid, nxt, cnt, o[8:8 + 4 * OVF_CAP].view(np.int32).copy(),
                          o[8 + 4 * OVF_CAP:8 + 12 * OVF_CAP].view(np.float64).copy()))
            rem -= cnt
            oid = nxt
        rows.append(SimpleNamespace(y=y, nnz=nnz, first=first, idx=idx, val=val, chain=chain))
    return rows


# ---------------------------------------------------------------------------------------------------------------
# L_F
# ---------------------------------------------------------------------------------------------------------------

def gram_eigenvalues(x, standardize):
    """(lambda_1, lambda_2) of X'X / n -- of the centred, scaled features when standardised (what the solvers see)"""
    X = dense_of(x)
    if standardize:
        sd = X.std(axis=0)
        X = (X - X.mean(axis=0)) / np.where(sd == 0, 1.0, sd)
    w = np.linalg.eigvalsh(X.T @ X / X.shape[0])
    return float(w[-1]), float(w[-2])


# ---------------------------------------------------------------------------------------------------------------
# inputs: the smallest that reach each edge (the GPU test and the CPU proof of the bounds use the same ones)
# ---------------------------------------------------------------------------------------------------------------

def _values(rng, k):
    return rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k)


def _from_columns(rng, n, col_nnz):
    X = np.zeros((n, len(col_nnz)))
    for j, k in enumerate(col_nnz):
        X[rng.choice(n, k, replace=False), j] = _values(rng, k)
    return X


def _from_rows(rng, p, row_nnz):
    X = np.zeros((len(row_nnz), p))
    for i, k in enumerate(row_nnz):
        X[i, rng.choice(p, k, replace=False)] = _values(rng, k)
    return X


def sparse_column_cases():
    """name -> dense array.  Column lengths 0, 1, 255, 256, 257 and 600 around the 256-thread block-strided loops and
    block_sum's four wavefronts; a full column of the constant 3.0 at n = 512; p = 1."""
    rng = np.random.default_rng(20240)
    lens = _from_columns(rng, 640, [0, 1, 255, 256, 257, 600, 40, 3])
    const = _from_columns(rng, 512, [30, 512, 100])
    const[:, 1] = 3.0
    return {"column_lengths": lens, "constant_column": const, "one_column": _from_columns(rng, 50, [17])}


ROW_EDGE_LENGTHS = [0, 1, 13, 14, 15, 19, 20, 21, 34, 35, 40, 41, 63, 64, 65, 512, 530]


def sparse_row_cases():
    """name -> dense array.  short_rows: more than 90 % of the rows have fewer than 64 entries (the percentile sets the
    cap: 14 at rec_align 64, 20 at 128 and 256) and the rest are cap - 1, cap, cap + 1, cap + 20, cap + 21 for both
    caps, 63 / 64 / 65 around the histogram's last bin, and 512 / 530 around the largest cap.  long_rows: they are
    not, so the cap is min(longest row, 512), grown into the slack; long_rows_100 the same with a longest row of 100."""
    rng = np.random.default_rng(20241)
    p = 600
    short = _from_rows(rng, p, ROW_EDGE_LENGTHS + [int(k) for k in rng.integers(0, 13, 283)])
    long_ = _from_rows(rng, p, [int(k) for k in rng.integers(64, 101, 30)] + [512, 530, 0, 1, 20, 63, 64, 65])
    return {"short_rows": short, "long_rows": long_, "long_rows_100": long_[:30].copy()}


SPARSE_N = [1, 2, 255, 256, 257, 1024, 1025]


def sparse_n_case(n):
    """n x 7, about a third of the entries stored; end_bit of the radix sort at and just past a power of two, the
    grid-stride tails of the per-sample kernels"""
    rng = np.random.default_rng(3000 + n)
    X = _values(rng, n * 7).reshape(n, 7) * (rng.random((n, 7)) < 0.35)
    X[0, 0] = 1.25                            # never an empty matrix
    return X


DENSE_SHAPES = [(1, 33), (31, 64), (32, 257), (33, 1), (63, 32), (64, 31), (65, 63), (257, 65)]


def dense_case(n, p):
    """the 32 x 32 transpose tiles and the 64-lane row norm below, at and above their edges; non-square"""
    rng = np.random.default_rng(100 * n + p)
    return rng.standard_normal((n, p)) * rng.uniform(0.5, 3.0, p) + rng.uniform(-1.0, 1.0, p)


def ymap_for(n, cols, seed=7):
    return np.random.default_rng(seed + 31 * n + cols).standard_normal((n, cols))


def l_f_case():
    """Non-negative sparse data with a common component that survives centring: the rows differ in how many entries
    they hold (2 % or 60 % of the features), so all features are positively correlated.  2000 x 120."""
    rng = np.random.default_rng(20242)
    n, p = 2000, 120
    dens = np.where(rng.random(n) < 0.2, 0.6, 0.02)
    return rng.uniform(0.0, 1.0, (n, p)) * (rng.random((n, p)) < dens[:, None])


def l_f_truth(x, standardize):
    """lambda_1, after confirming the gap the stop rule's deficit bound needs: lambda_2 / lambda_1 <= 0.5"""
    l1, l2 = gram_eigenvalues(x, standardize)
    assert l2 / l1 <= 0.5, (l1, l2)
    return l1
