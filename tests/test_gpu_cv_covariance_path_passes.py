"""The path kernels of the cross-validations of the covariance family (covariance_cv_run and mcovariance_cv_run: cov_path_kernel
and cov_group_path_kernel over a grid of jobs; wcovariance_cv_run and wmcovariance_cv_run: cov_wide_cv_path_kernel and
cov_wide_group_cv_path_kernel) job by job, through sgdnet_cv_covariance_probe, against tests/covariance_path_reference.py.
tests/test_gpu_cv_covariance_passes.py checks the stages BEFORE the path kernel.

3 groups of different sizes (so that n_T differs between the sets) x 2 mixes, one of them 0 (so that ridge_jobs differs between
the jobs): 6 jobs, with train_on = "fold" and "rest", one shape per form with p odd.  What is under test is the job
arithmetic: job = mix * n_sets + set reads set job % n_sets and its OWN penalties, functor and output slices.  So every job is
held to checks A, B, C and E against ITS training set's tapped inputs (Mt, scale and n_T, or S, diag S and c~) and ITS tapped
pen_a, pen_b and ridge, with the tol and max_iter the kernel was handed (tapped too: the probe goes through fit_cv_*, which
takes them from sgdnet_control).
A job's W against a single fit: the single-fit probe takes x and y, not moments, so it cannot be handed a job's tapped
inputs; instead every job's one-sweep W and G are held to the float64 restatement run on the job's own tapped inputs, within
twice check D's bound, and to the long-double replay within the bound itself."""
import numpy as np
import pytest

import covariance_path_reference as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    import torch  # noqa: F401  -- before libsgdnet_hip.so (sgdnet_amd/_lib.py)
    import sgdnet_amd
    if sgdnet_amd.load().sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    from sgdnet_amd import diagnostics
    return diagnostics


@pytest.mark.parametrize("form,n,p,K", P.CV_FORMS)
@pytest.mark.parametrize("train_on", ["fold", "rest"])
def test_every_job_against_its_own_set_and_penalties(probe, form, n, p, K, train_on):
    case = P.cv_case(form, n, p, K)
    y = P.cv_response(case)

    def run(tol, max_iter):
        o = probe.cv_covariance_probe(case.x, y, case.fold, P.CV_GROUPS, case.mixes, case.lams, train_on=train_on, wide=case.wide, maxit=max_iter,
                                      thresh=tol)
        assert o.tol[0] == tol and o.max_iter[0] == max_iter, "the kernel was handed another stopping rule than the control block's"
        assert o.W.shape == (len(case.mixes), P.CV_GROUPS, case.lams.shape[1], p, K) and o.sweeps.dtype == np.int64
        if case.wide:
            P.check_pad(o.S)
        return o

    def fields_of(o):
        assert np.array_equal(o.ridge, np.repeat((case.mixes == 0.0)[:, None], P.CV_GROUPS, axis=1)), "ridge_jobs"
        assert len(set(o.tstat[0])) == P.CV_GROUPS, "the training sets have different sizes"
        return P.cv_device_models(case, o), o.pen_a, o.pen_b, o.ridge

    P.check_cv(case, run, fields_of, what=f"cv {form} {train_on}")
