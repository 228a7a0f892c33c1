"""Cross-validation in wide multinomial Newton mode (sgdnet_cv_wmnewton_*, sa.cv_wmnewton_fits) and its option
"cv_wmnewton_moments" on the CPU: the new names in all three layers, the option's values, the refusals decided before a device
is looked for, and mnewton.hpp's wmnewton_cv_bytes against its restatement.  Also what tests/test_gpu_cv_wmnewton.py shares with
this file: its EDGES, their inputs, and the float64 restatement of a job stopped after exactly two Newton steps."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import cv_mnewton_reference as ref
import test_gpu_cv_covariance as tcv
import test_gpu_mnewton as tm
import wmnewton_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET_BYTES = 16 << 30                    # mnewton.hpp: kWmnewtonCvBytes

# (n, p, K, folds, mixes, train_on): see tests/test_gpu_cv_wmnewton.py
EDGES = [(513, 62, 2, 2, 1, "fold"), (513, 62, 2, 2, 3, "fold"), (450, 63, 3, 3, 2, "rest"), (390, 62, 4, 3, 2, "rest"),
         (385, 127, 2, 3, 2, "rest")]
TWO_STEP_EDGES = [EDGES[0], EDGES[2]]
TWO_STEP = dict(mix=0.0, lam=np.array([0.05]), standardize=False, thresh=wr.THRESH, maxit=2)


def mixes_of(count):
    return [0.5] if count == 1 else list(np.linspace(0.0, 1.0, count))


def edge_input(edge, seed=1):
    """x, y, foldid of an edge; every training set holds every class (asserted: the seed was picked so that it does)"""
    n, p, K, folds = edge[:4]
    x, y = tm.problem(n, p, K, False, seed=seed)
    return x, y, ref.equal_folds(n, folds, y, K, seed=seed)


def edge_lambdas(edge, x, y, mix):
    """a short automatic path of the whole data, by the rule wmnewton_reference has for the rows of the smallest training set"""
    n, p, K, folds = edge[:4]
    n_t = n // folds if edge[5] == "fold" else n - (n + folds - 1) // folds
    nlambda, ratio = wr.path_of((n_t, p, K), mix)
    return wr.automatic_lambdas(x, y, K, mix, True, nlambda, ratio)


def two_step_reference(edge):
    """per training set the float64 restatement of the job stopped after two Newton steps: (a0, beta, dev_ratio, info)"""
    x, y, foldid = edge_input(edge)
    kw = {k: v for k, v in TWO_STEP.items() if k not in ("mix", "lam")}
    return x, y, foldid, [wr.numpy_wide_mnewton_path(x[T], y[T], edge[2], TWO_STEP["lam"], TWO_STEP["mix"], **kw)
                          for T in tcv.training_sets(foldid, edge[5])]


def mfma_chunks(n_t, p, K):
    """mnewton.hpp: wmnewton_mfma_row_chunks"""
    tiles = (p + 2 + 63) // 64
    workgroups = tiles * (tiles + 1) // 2 * ((K * (K + 1) // 2 + 5) // 6)
    cap = 1 if workgroups >= 2048 else 2048 // workgroups
    rows = max(256, ((n_t + cap - 1) // cap + 31) // 32 * 32)
    return (n_t + rows - 1) // rows


def workspace_bytes(n_mix, n_t, n, p, K, n_lambda, mfma):
    """mnewton.hpp: wmnewton_cv_workspace_bytes, restated.  n_t: the rows of each training set"""
    pairs, Q = K * (K + 1) // 2, K * (p + 1)
    chunks = max((mfma_chunks if mfma else wr.row_chunks)(t, p, K) for t in n_t)
    tiles = (p + 2 + 63) // 64
    tile = tiles * (tiles + 1) // 2 * 4096 if mfma else wr.tile_pairs(p + 2) * 256
    per_job = pairs * (p + 2) ** 2 + chunks * pairs * tile + (Q + 15) // 16 * 16 * Q + 2 * Q + 1024 + 3 * Q + 8 + n_lambda * Q
    return 8 * (n_mix * sum(n_t) * K + n_mix * len(n_t) * per_job + n * p + n)


def test_header_binding_and_package_agree():
    import sgdnet_amd as sa
    from sgdnet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sgdnet_hip.h")).read()
    for name in ("sgdnet_cv_wmnewton_dense", "sgdnet_cv_wmnewton_sparse"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in _lib.EXPORTS and hasattr(sa.load(), name), name
    for name in ("cv_wmnewton_fits", "cv_sgdnet_wmnewton"):
        assert name in sa.__all__ and callable(getattr(sa, name)), name
    assert re.search(r"typedef sgdnet_cv_mnewton_result sgdnet_cv_wmnewton_result;", hdr)
    narrow = re.search(r"int sgdnet_cv_mnewton_dense\((.*?)\);", hdr, re.S).group(1)
    wide = re.search(r"int sgdnet_cv_wmnewton_dense\((.*?)\);", hdr, re.S).group(1)
    assert " ".join(narrow.split()).replace("sgdnet_cv_mnewton_result", "sgdnet_cv_wmnewton_result") == " ".join(wide.split())
    L = sa.load()
    for kind in ("dense", "sparse"):
        assert [str(t) for t in getattr(L, "sgdnet_cv_wmnewton_" + kind).argtypes] == [str(t) for t in getattr(L, "sgdnet_cv_mnewton_" + kind).argtypes]


def test_option_is_in_the_header_and_takes_0_and_1_only():
    import sgdnet_amd as sa
    assert '"cv_wmnewton_moments"' in open(os.path.join(ROOT, "include", "sgdnet_hip.h")).read()
    assert sa.get_option("cv_wmnewton_moments") == 0
    for value in (1, 0):
        with sa.option("cv_wmnewton_moments", value):
            assert sa.get_option("cv_wmnewton_moments") == value
    for value in (2, -1):
        with pytest.raises(sa.SgdnetError):
            sa.set_option("cv_wmnewton_moments", value)
    assert sa.get_option("cv_wmnewton_moments") == 0


def test_workspace_arithmetic_is_the_headers():
    """the worked examples mnewton.hpp asserts, from the restatement: 50 jobs at 2000 x 1000, K = 3 under both options, and the
    jobs that fit at K = 2's feature limit"""
    hpp = open(os.path.join(ROOT, "sgdnet_amd", "csrc", "mnewton.hpp")).read()
    assert "constexpr size_t wmnewton_cv_bytes(" in hpp and hpp.count("wmnewton_cv_bytes(5, 10, 18000, 2000, 1000, 3, 100,") >= 3
    assert re.search(r"kWmnewtonCvBytes = kWnewtonCvBytes;", hpp) and "kWmnewtonCvMfmaGroup = 6;" in hpp
    folds = [1800] * 10
    assert wr.row_chunks(1800, 1000, 3) == 1 and mfma_chunks(1800, 1000, 3) == 8
    assert workspace_bytes(5, folds, 2000, 1000, 3, 100, False) // 10 ** 7 == 740
    assert workspace_bytes(5, folds, 2000, 1000, 3, 100, True) // 10 ** 7 == 1686 and workspace_bytes(5, folds, 2000, 1000, 3, 100, True) <= BUDGET_BYTES
    limit = wr.max_features(2)
    for mfma in (False, True):
        assert workspace_bytes(29, [2000], 2000, limit, 2, 100, mfma) <= BUDGET_BYTES < workspace_bytes(30, [2000], 2000, limit, 2, 100, mfma)


def test_native_refusals_name_the_condition():
    """every one of them is decided before any HIP call: they are the same with and without a device"""
    import sgdnet_amd as sa
    rng = np.random.default_rng(0)
    x = rng.standard_normal((60, 4))
    y = np.digitize(x[:, 0] + rng.standard_normal(60), [-0.5, 0.5]).astype(float)
    fold = np.arange(60) % 3

    def refused(code, needle, xx, yy, ff, alpha=0.5, **kw):
        with pytest.raises(sa.SgdnetError) as e:
            sa.cv_wmnewton_fits(xx, yy, ff, alpha, [[0.1, 0.01]] * np.size(alpha) if np.ndim(alpha) else [0.1, 0.01], **kw)
        assert e.value.code == code and needle in str(e.value), str(e.value)

    few, few_cls = np.arange(18) % 3, (np.arange(18) // 3 % 3).astype(float)      # every group of six rows holds two of each class
    limit = sa.wmnewton_max_features(3)
    wide = rng.standard_normal((18, limit + 1))
    refused(-5, "cv wmnewton needs no more features than sgdnet_wmnewton_max_features(n_classes)", wide, few_cls, few)
    # the dense copy of a sparse x: 70 000 x 2000 x 8 bytes > 1 GiB (nothing is stored, so nothing that large is made)
    tall_cls = (np.arange(70_000) % 2).astype(float)                    # (two classes: 2000 features are within their limit)
    refused(-5, "cv wmnewton needs the dense copy of a sparse x", sp.csc_matrix((70_000, 2000)), tall_cls, np.arange(70_000) // 2 % 3)
    # the workspace: at K = 2's feature limit a job is 0.58 GB; 9 mixes x 3 folds = 27 jobs fit the 16 GiB, 10 x 3 do not
    two, two_cls = np.arange(12) % 3, (np.arange(12) // 3 % 2).astype(float)
    at_limit = rng.standard_normal((12, wr.max_features(2)))
    n_t = [4, 4, 4]
    assert workspace_bytes(9, n_t, 12, at_limit.shape[1], 2, 2, False) <= BUDGET_BYTES < workspace_bytes(10, n_t, 12, at_limit.shape[1], 2, 2, False)
    for setting in (0, 1):
        with sa.option("cv_wmnewton_moments", setting):
            refused(-5, "cv wmnewton needs the jobs' workspace within %d bytes: 10 mixes x 3 groups of 12 rows" % BUDGET_BYTES, at_limit, two_cls,
                    two, alpha=list(np.linspace(0, 1, 10)))
            refused(-5, "are %d bytes" % workspace_bytes(10, n_t, 12, at_limit.shape[1], 2, 2, bool(setting)), at_limit, two_cls, two,
                    alpha=list(np.linspace(0, 1, 10)))
    # jobs x class pairs beyond a grid dimension: 99 classes are 4950 pairs, 7 mixes x 2 groups are 14 jobs
    many_cls = np.repeat(np.arange(99), 4).astype(float)
    refused(-5, "cv wmnewton needs no more than 65535 jobs, 65535 jobs x class pairs", rng.standard_normal((396, 3)), many_cls, np.arange(396) % 2,
            alpha=list(np.linspace(0, 1, 7)))
    # a training set without a class: group 0 holds the rows of class 0 and nothing else
    order, first = np.argsort(y, kind="stable"), int((y == 0).sum())
    missing = fold.copy()
    missing[order[:first]] = 0
    missing[order[first:]] = 1 + np.arange(60 - first) % 2
    refused(-1, "the training set of group 0 of 3 holds no row of class 1", x, y, missing)
    with sa.option("wmnewton_width", 512):
        refused(-1, "wmnewton_width", x, y, fold)
