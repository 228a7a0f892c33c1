"""CPU proof that the bounds of tests/setup_reference.py admit any legal summation order, on every input
tests/test_gpu_setup_passes.py gives the device: the setup passes' arithmetic is carried out in float64 with the sums
taken sequentially, pairwise, and as 256 strided partial sums (the kernels' own shape), and all three must stay inside
the bounds around the long-double truth.  Also pins the restated record geometry and the decoder on hand-made cases."""
import numpy as np
import pytest

import setup_reference as R


def seq_sum(t):
    return float(np.add.accumulate(np.asarray(t, dtype=np.float64))[-1]) if len(t) else 0.0


def pair_sum(t):
    t = np.asarray(t, dtype=np.float64)
    if len(t) <= 2:
        return seq_sum(t)
    h = len(t) // 2
    return pair_sum(t[:h]) + pair_sum(t[h:])


def strided_sum(t):
    t = np.asarray(t, dtype=np.float64)
    return pair_sum([seq_sum(t[i::256]) for i in range(min(256, len(t)))])


SUMS = {"sequential": seq_sum, "pairwise": pair_sum, "strided256": strided_sum}


def float64_passes(x, ymap, standardize, sparse, fsum):
    """col_stats / xt_times / row_norm (sparse) or their dense_* counterparts in float64, every sum through fsum"""
    X = R.dense_of(x)
    n, p = X.shape
    Y = np.asarray(ymap, dtype=np.float64).reshape(n, -1)
    center, scale, msq = np.zeros(p), np.ones(p), np.zeros(p)
    xty = np.zeros((p, Y.shape[1]))
    H = np.zeros((n, p))                       # the values the passes hold
    for j in range(p):
        st = X[:, j] != 0 if sparse else np.ones(n, dtype=bool)
        v = X[st, j]
        held = v
        if standardize:
            mean = fsum(v) / n
            dlt = v - mean
            if sparse:
                var = fsum(dlt * dlt / n)
                var += (n - len(v)) * mean * mean / n
            else:
                var = fsum(dlt * dlt) / n
            sd = 1.0 if var == 0.0 else float(np.sqrt(var))
            held = v / sd if sparse else dlt / sd
            center[j], scale[j] = mean, sd
        H[st, j] = held
        msq[j] = fsum(held * held) / n
        for c in range(Y.shape[1]):
            xty[j, c] = fsum(held * Y[st, c])
    best = 0.0
    cs = center / scale
    csq = fsum(cs * cs)
    for i in range(n):
        st = X[i] != 0 if sparse else np.ones(p, dtype=bool)
        if sparse and standardize:
            d = H[i, st] - cs[st]
            nrm = fsum(d * d) + (csq - fsum(cs[st] * cs[st]))
        else:
            nrm = fsum(H[i, st] * H[i, st])
        best = max(best, nrm)
    return center, scale, msq, xty, best


def _inside(got, exact, bound, what):
    err = np.abs(np.asarray(got, dtype=R.LD) - exact)
    assert np.all(err <= bound), f"{what}: error {float(err.max()):.3e} outside the bound {float(np.max(bound)):.3e}"


def _check_case(x, cols, standardize, sparse):
    ymap = R.ymap_for(x.shape[0], cols)
    B = R.moment_bounds(x, ymap, standardize, sparse)
    for name, fsum in SUMS.items():
        center, scale, msq, xty, best = float64_passes(x, ymap, standardize, sparse, fsum)
        _inside(center, B.exact.mean, B.center, f"{name} mean")
        _inside(scale, B.exact.sd, B.scale, f"{name} sd")
        _inside(msq, B.exact.mean_sq, B.mean_sq, f"{name} mean_sq")
        _inside(xty, B.exact.xty, B.xty, f"{name} x'y")
        _inside(best, B.exact.max_sqnorm, B.max_sqnorm, f"{name} max_sqnorm")
    # the bounds are rounding-error bounds, not tolerances: a wrong 9th digit must not fit
    nc = ~R.constant_columns(x)
    if standardize and nc.any():
        assert float(np.max(B.scale[nc] / B.exact.sd[nc])) < 1e-9
        assert float(np.max(B.center[nc] / B.exact.sd[nc])) < 1e-9
    assert float(B.mean_sq.max()) <= 1e-9 * max(1.0, float(B.exact.mean_sq.max()))
    assert float(B.xty.max()) <= 1e-9 * max(1.0, float(np.abs(B.exact.xty).max()))
    assert float(B.max_sqnorm) <= 1e-9 * max(1.0, float(B.exact.max_sqnorm))


SPARSE_INPUTS = {**R.sparse_column_cases(), **R.sparse_row_cases(), **{f"n{n}": R.sparse_n_case(n) for n in R.SPARSE_N}}


@pytest.mark.parametrize("standardize", [0, 1])
@pytest.mark.parametrize("name", sorted(SPARSE_INPUTS))
def test_sparse_bounds_admit_every_summation_order(name, standardize):
    _check_case(SPARSE_INPUTS[name], 3 if name in ("column_lengths", "n257") else 1, standardize, True)


@pytest.mark.parametrize("standardize", [0, 1])
@pytest.mark.parametrize("n,p", R.DENSE_SHAPES)
def test_dense_bounds_admit_every_summation_order(n, p, standardize):
    _check_case(R.dense_case(n, p), 3 if n == 65 else 1, standardize, False)


def test_constant_column_has_sd_exactly_one_in_every_order():
    x = R.sparse_column_cases()["constant_column"]
    for fsum in SUMS.values():
        center, scale, _msq, _xty, _best = float64_passes(x, R.ymap_for(512, 1), 1, True, fsum)
        assert center[1] == 3.0 and scale[1] == 1.0


def test_an_inexact_constant_column_is_refused():
    x = np.full((10, 2), 0.1)
    with pytest.raises(AssertionError):
        R.constant_columns(x)


def test_l_f_inputs_have_the_gap_the_stop_rule_needs():
    x = R.l_f_case()
    assert x.min() >= 0.0 and x.shape[0] <= 5000 and x.shape[1] <= 200
    for standardize in (0, 1):
        l1, l2 = R.gram_eigenvalues(x, standardize)
        assert l2 / l1 <= 0.5
        rho2 = (l2 / l1) ** 2
        assert rho2 / (1 - rho2) * 2e-3 < 1e-3          # the deficit the stop rule can leave
        assert R.l_f_truth(x, standardize) == l1


def test_record_geometry_rule_on_hand_made_histograms():
    # 90 % of 100 rows have <= 10 entries: 16 + 40 + 80 = 136 bytes -> 256 at 128-B alignment, which holds 20
    z = [10] * 95 + [70] * 5
    g = R.record_geometry(z, 128)
    assert (g.stride, g.cap, g.val_off) == (256, 20, 16 + 80) and g.n_ovf == 5 * 3 and list(g.blocks[-5:]) == [3] * 5
    g = R.record_geometry(z, 64)
    assert (g.stride, g.cap, g.val_off) == (192, 14, 16 + 56)
    g = R.record_geometry(z, 256)
    assert (g.stride, g.cap) == (256, 20)
    # the percentile row has 64 or more entries: the longest row, at most 512, grown into the slack
    g = R.record_geometry([80] * 50 + [600], 128)
    assert g.cap == 521 and g.stride == 6272 and g.val_off == 16 + 2088 and g.n_ovf == 4
    g = R.record_geometry([80] * 50 + [100], 128)
    assert g.stride == 1280 and g.cap == 105 and g.n_ovf == 0
    # empty rows only: the cap is at least 1; a single row: want = 0 is met by the first bin
    assert R.record_geometry([0] * 10, 128).cap == 9 and R.record_geometry([0] * 10, 128).stride == 128
    assert R.record_geometry([5], 64).cap == 4 and R.record_geometry([5], 64).n_ovf == 1
    for c in range(1, 600):
        assert R.rec_bytes(c) % 8 == 0


def test_decoder_round_trips_a_hand_packed_record():
    cap, stride = 4, 64
    val_off = 16 + 16
    rec = np.zeros(2 * stride, dtype=np.uint8)
    ovf = np.zeros(2 * R.OVF_STRIDE, dtype=np.uint8)
    rec[0:8].view(np.float64)[0] = 1.5
    rec[8:16].view(np.int32)[:] = (2, 0)
    rec[16:32].view(np.int32)[:] = (3, 9, 0, 0)
    rec[val_off:val_off + 32].view(np.float64)[:] = (0.5, -2.0, 0.0, 0.0)
    b = rec[stride:]
    b[8:16].view(np.int32)[:] = (4 + 20 + 1, 0)
    b[16:32].view(np.int32)[:] = (1, 2, 3, 4)
    b[val_off:val_off + 32].view(np.float64)[:] = (1, 2, 3, 4)
    for k, cnt in ((0, 20), (1, 1)):
        o = ovf[k * R.OVF_STRIDE:]
        o[0:8].view(np.int32)[:] = (k + 1, cnt)
        o[8:8 + 4 * cnt].view(np.int32)[:] = np.arange(10, 10 + cnt)
        o[88:88 + 8 * cnt].view(np.float64)[:] = np.arange(cnt) + 0.25
    rows = R.decode_records(rec, ovf, 2, stride, cap, val_off)
    assert rows[0].y == 1.5 and rows[0].nnz == 2 and rows[0].chain == [] and list(rows[0].idx) == [3, 9, 0, 0]
    assert rows[1].nnz == 25 and [(c[0], c[1], c[2]) for c in rows[1].chain] == [(0, 1, 20), (1, 2, 1)]
    assert list(rows[1].chain[1][3][:2]) == [10, 0] and rows[1].chain[0][4][19] == 19.25


def test_sample_major_is_scipy_csr_with_sorted_indices():
    import scipy.sparse as sp
    x = sp.csc_matrix(R.sparse_n_case(257))
    sptr, sidx, pos = R.sample_major(x)
    csr = x.tocsr()
    csr.sort_indices()
    assert np.array_equal(sptr, csr.indptr) and np.array_equal(sidx, csr.indices) and np.array_equal(x.data[pos], csr.data)
    for i in range(257):
        assert np.all(np.diff(sidx[sptr[i]:sptr[i + 1]]) > 0)
