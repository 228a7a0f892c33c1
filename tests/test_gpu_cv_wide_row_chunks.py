"""The wide cross-validations (wcovariance_cv_run, wmcovariance_cv_run) with dense x and a group that spans two row chunks of the
group moments pass: the case the shapes of tests/test_gpu_cv_wcovariance.py and tests/test_gpu_cv_wmcovariance.py leave out
(their groups have at most 220 rows and a chunk never fewer than 256 there; the narrow CVs' tests have groups of 400 rows in
chunks of 256).  Each case is that file's own check (check_jobs: KKT on x[T], y[T] and the separate fit of every job) at that
file's bounds.

Up to 256 rows the pass has one row chunk, whatever the columns.  257 rows over the fewest columns the entry points take (one
feature; p + 2 or p + K + 1 columns are one tile pair) are cut every ceil(257 / 2) = 129 -> 192 rows (whole 64-row steps), so a
group of 200 rows is two chunks whose partial tiles cov_reduce_kernel adds, and the other 57 rows are a third."""
import numpy as np
import pytest

import cv_wcovariance_reference as cw
import cv_wmcovariance_reference as cwm
import test_gpu_cv_wcovariance as tw
import test_gpu_cv_wmcovariance as twm

pytestmark = pytest.mark.gpu

N, P, K = 257, 1, 2
SIZES = [200, 57]
SEED = 12                      # (a seed at which the one feature carries signal in both generators)


@pytest.fixture(scope="module")
def sa():
    import torch  # noqa: F401
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    return sgdnet_amd


def folds():
    return np.repeat([1, 2], SIZES)[np.random.default_rng(9).permutation(N)]


@pytest.mark.parametrize("train_on", ["fold", "rest"])
def test_wcovariance_group_spans_two_row_chunks(sa, train_on):
    assert cw.rows_per_chunk(N - 1, P + 2) == N - 1 and cw.rows_per_chunk(N, P + 2) == 192 and cw.row_chunks(N, P, SIZES) == 3
    x, y = cw.problem(N, P, False, seed=SEED)
    tw.check_jobs(sa, x, y, folds(), cw.MIXES, train_on)


@pytest.mark.parametrize("train_on", ["fold", "rest"])
def test_wmcovariance_group_spans_two_row_chunks(sa, train_on):
    assert cwm.rows_per_chunk(N - 1, P + K + 1) == N - 1 and cwm.rows_per_chunk(N, P + K + 1) == 192 and cwm.row_chunks(N, P, K, SIZES) == 3
    x, y = cwm.problem(N, P, K, False, seed=SEED)
    twm.check_jobs(sa, x, y, folds(), cwm.MIXES, train_on)
