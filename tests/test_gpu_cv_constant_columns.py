"""A column that is constant on a training set and not on the data, through the four batched
cross-validations of the covariance family: one regression test each for cv_covariance_fits, cv_mcovariance_fits,
cv_wcovariance_fits and cv_wmcovariance_fits, with the helpers, the KKT bound and the SAME_OPTIMUM of that mode's own module
(tests/test_gpu_cv_covariance.py, _mcovariance, _wcovariance, _wmcovariance: check_jobs holds every job to KKT <= 1e-8 lambda
on x[T], y[T] and to 1e-9 of the separate fit).

The input: an indicator that is 1 on rows of fold 1 only, so that the other two training sets (train_on = "fold") see it all
0.  Re-centred from the whole-data mean its variance there is rounding noise about 0 of either sign; the kernels used to
ask "> 0" and could take the noise for an sd of 1e-8 (tests/test_gpu_cv_covariance_passes.py has the stage-by-stage view).
With the rule the column is constant: a coefficient of exactly 0 on those jobs -- the ridge functor (mix 0) included, which
has no threshold to hide a spurious coefficient behind -- and every job the optimum of the separate fit."""
import numpy as np
import pytest

import cv_wcovariance_reference as crw
import cv_wmcovariance_reference as crm
import test_gpu_cv_covariance as tcc
import test_gpu_cv_mcovariance as tcm
import test_gpu_cv_wcovariance as tcw
import test_gpu_cv_wmcovariance as tcwm

pytestmark = pytest.mark.gpu

MIXES = [0.0, 0.5]
G = 3


@pytest.fixture(scope="module")
def sa():
    import torch  # noqa: F401
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    return sgdnet_amd


def with_indicator(x):
    """column 1 becomes the indicator; three folds of 30 rows in row order"""
    x[:, 1] = 0.0
    x[np.random.default_rng(9).choice(30, 11, replace=False), 1] = 1.0
    return x, np.repeat([1, 2, 3], 30)


def indicator_is_out(fits, several):
    first = fits[0].beta                            # mix 0, the set where the column varies: a feature like any other
    assert np.all((np.stack(first) if several else first)[..., 1, :] != 0.0)
    for a in range(len(MIXES)):
        for j in (1, 2):
            beta = fits[a * G + j].beta
            for b in (beta if several else [beta]):
                assert np.all(b[1] == 0.0), (MIXES[a], j, b[1])


def test_covariance(sa):
    x, y = tcc.problem(90, 6, False, seed=9)
    x, foldid = with_indicator(x)
    indicator_is_out(tcc.check_jobs(sa, x, y, foldid, MIXES, "fold"), False)


def test_mcovariance(sa):
    x, y = tcm.problem(90, 6, 3, False, seed=9)
    x, foldid = with_indicator(x)
    indicator_is_out(tcm.check_jobs(sa, x, y, foldid, MIXES, "fold"), True)


def test_wcovariance(sa):
    x, y = crw.problem(90, 205, False, seed=9)
    x, foldid = with_indicator(x)
    indicator_is_out(tcw.check_jobs(sa, x, y, foldid, MIXES, "fold"), False)


def test_wmcovariance(sa):
    x, y = crm.problem(90, 205, 3, False, seed=9)
    x, foldid = with_indicator(x)
    indicator_is_out(tcwm.check_jobs(sa, x, y, foldid, MIXES, "fold"), True)
