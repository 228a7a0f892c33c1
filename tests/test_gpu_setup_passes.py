"""The device setup passes (sgdnet_amd/csrc/setup_device.hip) one by one, through sgdnet_setup_probe_sparse / _dense,
against exact references (tests/setup_reference.py).

Exact, bit for bit: the sample-major form (scipy's CSR with sorted indices: the radix sort is stable inside a row),
sval = raw / scale and dense xt = (x - center) / scale with the DEVICE's own center and scale (one and two IEEE
operations), dense_sample_rows, the record geometry, and every field of every packed record and overflow record.

Bounded: center, scale, mean_sq, x'y and max_sqnorm against the long-double truth, inside the rounding-error bounds
that setup_reference.moment_bounds composes over the kernels' own arithmetic (mean -> deviation -> square -> divide ->
sqrt; a double sum of m terms in any order errs by at most gamma_m sum|t_i|; the derivation is in that module's
docstring).  tests/test_setup_reference.py shows on the CPU that sequential, pairwise and 256-strided float64 sums all
stay inside those bounds on these very inputs; none of them was taken from what a device returned.

L_F: |A v| <= lambda_1 for a unit v, so L_F <= lambda_1 on any input; with lambda_2 / lambda_1 <= 0.5 (checked on the
CPU) the stop rule (relative change <= 2e-3 after >= 4 iterations) leaves a deficit below 1e-3."""
import numpy as np
import pytest
import scipy.sparse as sp

import setup_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    import torch  # noqa: F401  -- before libsgdnet_hip.so (sgdnet_amd/_lib.py)
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    from sgdnet_amd import diagnostics
    return diagnostics


def _inside(got, exact, bound, what):
    err = np.abs(np.asarray(got, dtype=R.LD) - exact)
    worst = int(np.argmax(err - bound)) if np.ndim(err) else 0
    print(f"{what}: largest error {float(np.max(err)):.3e}, bound there {float(np.ravel(bound)[worst]):.3e}")
    assert np.all(err <= bound), f"{what}: error {float(np.ravel(err)[worst]):.3e} outside {float(np.ravel(bound)[worst]):.3e}"


def _check_moments(o, x, ymap, standardize, sparse):
    B = R.moment_bounds(x, ymap, standardize, sparse)
    const = R.constant_columns(x)
    _inside(o.center, B.exact.mean, B.center, "center")
    _inside(o.scale, B.exact.sd, B.scale, "scale")
    if standardize:
        assert np.all(o.scale[const] == 1.0)                   # variance exactly 0 -> exactly 1
    else:
        assert np.all(o.center == 0.0) and np.all(o.scale == 1.0)
    j = int(np.argmax(B.exact.mean_sq))
    # max_mean_sq is the largest of p values: |max a - max b| <= max |a - b|
    _inside(o.max_mean_sq, B.exact.mean_sq[j], B.mean_sq.max(), "max_mean_sq")
    _inside(o.xty, B.exact.xty, B.xty, "x'y")
    _inside(o.max_sqnorm, B.exact.max_sqnorm, B.max_sqnorm, "max_sqnorm")


def _check_sample_major(o, xs):
    """sptr / sidx are scipy's; sval is the raw value over the device's own scale: one IEEE division"""
    sptr, sidx, pos = R.sample_major(xs)
    assert np.array_equal(o.sptr, sptr)
    assert np.array_equal(o.sidx, sidx)
    want = xs.data[pos] / o.scale[sidx]
    assert np.array_equal(o.sval, want)


def _check_records(o, xs, y, y_rows, rec_align):
    n = xs.shape[0]
    z = np.diff(o.sptr)
    g = R.record_geometry(z, rec_align)
    assert (o.rec_stride, o.rec_cap, o.rec_val_off, o.n_ovf) == (g.stride, g.cap, g.val_off, g.n_ovf)
    assert o.n_ovf == int(sum(-(-(int(k) - g.cap) // 20) for k in z if k > g.cap))
    assert len(o.rec) == n * g.stride and len(o.ovf) == 256 * g.n_ovf
    first = np.concatenate([[0], np.cumsum(g.blocks)])       # overflow ids are handed out in row order
    rows = R.decode_records(o.rec, o.ovf, n, g.stride, g.cap, g.val_off)
    seen = 0
    for i, r in enumerate(rows):
        q0, k = int(o.sptr[i]), int(z[i])
        idx, val = o.sidx[q0:q0 + k], o.sval[q0:q0 + k]
        assert r.nnz == k and r.first == first[i], i
        assert r.y == (y[0, i] if y_rows == 1 else 0.0), i
        c0 = min(k, g.cap)
        assert np.array_equal(r.idx[:c0], idx[:c0]) and np.array_equal(r.val[:c0], val[:c0]), i
        assert np.all(r.idx[c0:] == 0) and np.all(r.val[c0:] == 0.0), f"row {i}: padding lanes"
        assert np.all(np.signbit(r.val[c0:]) == 0)
        assert len(r.chain) == g.blocks[i], i
        done = c0
        for b, (oid, nxt, cnt, oi, ov) in enumerate(r.chain):
            assert oid == first[i] + b and nxt == oid + 1 and cnt == min(k - done, 20), (i, b)
            assert np.array_equal(oi[:cnt], idx[done:done + cnt]) and np.array_equal(ov[:cnt], val[done:done + cnt]), (i, b)
            assert np.all(oi[cnt:] == 0) and np.all(ov[cnt:] == 0.0), f"row {i} overflow {b}: padding lanes"
            done += cnt
            seen += 1
        assert done == k
    assert seen == g.n_ovf
    return g


def _sparse_probe(probe, x, cols, standardize, y_rows=1, rec_align=128):
    n = x.shape[0]
    xs = sp.csc_matrix(x)
    ymap = R.ymap_for(n, cols)
    y = np.random.default_rng(5 + n).standard_normal((y_rows, n))
    o = probe.setup_probe_sparse(xs, ymap, y, standardize=standardize, rec_align=rec_align)
    return o, xs, ymap, y


@pytest.mark.parametrize("standardize", [0, 1])
@pytest.mark.parametrize("name,cols", [("column_lengths", 3), ("constant_column", 1), ("one_column", 1)])
def test_sparse_column_passes(probe, name, cols, standardize):
    """columns of 0, 1, 255, 256, 257 and 600 entries; a full column of 3.0 (sd exactly 1, values untouched); p = 1"""
    x = R.sparse_column_cases()[name]
    o, xs, ymap, y = _sparse_probe(probe, x, cols, standardize)
    _check_moments(o, x, ymap, standardize, True)
    _check_sample_major(o, xs)
    _check_records(o, xs, y, 1, 128)
    if name == "constant_column":
        assert o.scale[1] == 1.0 and o.center[1] == (3.0 if standardize else 0.0)
        assert np.all(o.sval[o.sidx == 1] == 3.0)


@pytest.mark.parametrize("standardize", [0, 1])
@pytest.mark.parametrize("n", R.SPARSE_N)
def test_sparse_sample_counts(probe, n, standardize):
    """n = 1, 2, 255, 256, 257, 1024, 1025: the sort's end_bit at and past a power of two, the grid-stride tails"""
    x = R.sparse_n_case(n)
    o, xs, ymap, y = _sparse_probe(probe, x, 3 if n == 257 else 1, standardize, y_rows=3 if n == 256 else 1)
    _check_moments(o, x, ymap, standardize, True)
    _check_sample_major(o, xs)
    _check_records(o, xs, y, 3 if n == 256 else 1, 128)


@pytest.mark.parametrize("rec_align", [64, 128, 256])
@pytest.mark.parametrize("name", ["short_rows", "long_rows", "long_rows_100"])
def test_sparse_row_lengths_and_records(probe, name, rec_align):
    """rows of 0, 1, cap - 1 .. cap + 21, 63 / 64 / 65, 512 and 530 entries in one matrix; the percentile cap and the
    cap >= 64 branch; y inside the record (y_rows = 1) or not (3)"""
    x = R.sparse_row_cases()[name]
    y_rows = 3 if (name == "short_rows" and rec_align == 256) or name == "long_rows_100" else 1
    standardize = 1 if rec_align == 128 else 0
    o, xs, ymap, y = _sparse_probe(probe, x, 1, standardize, y_rows=y_rows, rec_align=rec_align)
    _check_sample_major(o, xs)
    g = _check_records(o, xs, y, y_rows, rec_align)
    z = set(int(k) for k in np.diff(o.sptr))
    if name == "short_rows":
        assert np.mean(np.diff(o.sptr) < 64) >= 0.9 and g.cap < 64
        assert {0, 1, g.cap - 1, g.cap, g.cap + 1, g.cap + 20, g.cap + 21, 63, 64, 65, 512, 530} <= z
    else:
        assert np.mean(np.diff(o.sptr) < 64) < 0.9 and g.cap >= min(max(z), 512)
    if rec_align == 128:
        _check_moments(o, x, ymap, standardize, True)


@pytest.mark.parametrize("standardize", [0, 1])
@pytest.mark.parametrize("n,p", R.DENSE_SHAPES)
def test_dense_passes(probe, n, p, standardize):
    """n, p in {1, 31, 32, 33, 63, 64, 65, 257}: the 32 x 32 transpose tiles and the 64-lane row norm at their edges"""
    x = R.dense_case(n, p)
    cols = 3 if n == 65 else 1
    ymap = R.ymap_for(n, cols)
    stride = 3
    m = (n + stride - 1) // stride
    o = probe.setup_probe_dense(x, ymap, standardize=standardize, sample_stride=stride, sample_m=m)
    _check_moments(o, x, ymap, standardize, False)
    # two IEEE operations with the device's own center and scale
    want = (x - o.center) / o.scale
    assert np.array_equal(o.xt, want)
    # dense_sample_rows reads the standardised column-major copy
    assert np.array_equal(o.sample, want[::stride][:m])


@pytest.mark.parametrize("standardize", [0, 1])
def test_l_f_is_the_largest_eigenvalue(probe, standardize):
    x = R.l_f_case()
    l1 = R.l_f_truth(x, standardize)
    n = x.shape[0]
    o = probe.setup_probe_sparse(sp.csc_matrix(x), np.zeros((n, 1)), np.zeros((1, n)), standardize=standardize)
    print(f"L_F {o.l_f:.12g}, lambda_1 {l1:.12g}, ratio {o.l_f / l1:.9f}")
    assert (1 - 2e-3) * l1 <= o.l_f <= l1 * (1 + 1e-10)


def test_probe_refuses_capacities_that_are_too_small(probe):
    import ctypes as C
    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    x = sp.csc_matrix(R.sparse_n_case(255))
    n, p = x.shape
    bufs = dict(center=np.empty(p), scale=np.empty(p), xty=np.empty(p), sval=np.empty(x.nnz))
    sptr, sidx = np.empty(n + 1, dtype=np.int64), np.empty(x.nnz, dtype=np.int32)
    rec, ovf = np.empty(64, dtype=np.uint8), np.empty(256, dtype=np.uint8)
    pr = _lib.SetupProbe()
    for k, v in bufs.items():
        setattr(pr, k, _lib.dptr(v))
    pr.sptr, pr.sidx = sptr.ctypes.data_as(C.POINTER(C.c_int64)), sidx.ctypes.data_as(C.POINTER(C.c_int32))
    pr.rec, pr.rec_bytes_cap, pr.ovf, pr.ovf_bytes_cap = rec.ctypes.data, rec.size, ovf.ctypes.data, ovf.size
    csc = _lib.Csc()
    csc.n_rows, csc.n_cols = n, p
    colptr, rowidx = x.indptr.astype(np.int32), x.indices.astype(np.int32)
    csc.colptr, csc.rowidx = colptr.ctypes.data_as(C.POINTER(C.c_int32)), rowidx.ctypes.data_as(C.POINTER(C.c_int32))
    csc.values = _lib.dptr(x.data)
    yz = np.zeros(n)
    rc = sa.load().sgdnet_setup_probe_sparse(C.byref(csc), 0, _lib.dptr(yz), 1, _lib.dptr(yz), 1, 128, 0, C.byref(pr))
    assert rc == -1 and b"capacities" in sa.load().sgdnet_last_error()
    assert pr.rec_stride == 128 and pr.n_ovf == 0                # the sizes a second call needs are reported
