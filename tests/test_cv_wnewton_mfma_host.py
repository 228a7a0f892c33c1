"""The option "cv_wnewton_moments" on the CPU (sgdnet_amd/csrc/newton_cv_mfma.hip: the matrix-core moments pass of the wide
Newton cross-validation): it is in the header, defaults to 0, takes 0 and 1 and refuses anything else; and the ridge penalty
tests/test_gpu_cv_wnewton_mfma.py stops its two-step cases at lets the restatement's inner solves converge."""
import os

import numpy as np
import pytest

import cv_wnewton_reference as cr
import test_gpu_newton as tn
import wnewton_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (n, p, folds, train_on): p + 2 = 64, 65, 129 -- one macro tile of 64 columns, a second that holds column p + 1 only, three
TWO_STEP_SHAPES = [(513, 62, 2, "fold"), (450, 63, 3, "rest"), (385, 127, 3, "rest")]
TWO_STEP = dict(mix=0.0, lam=np.array([0.05]), standardize=False, thresh=cr.THRESH, maxit=2)


def test_option_is_in_the_header_and_takes_0_and_1_only():
    import sgdnet_amd as sa
    assert '"cv_wnewton_moments"' in open(os.path.join(ROOT, "include", "sgdnet_hip.h")).read()
    assert sa.get_option("cv_wnewton_moments") == 0
    for value in (1, 0):
        with sa.option("cv_wnewton_moments", value):
            assert sa.get_option("cv_wnewton_moments") == value
    for value in (2, -1):
        with pytest.raises(sa.SgdnetError):
            sa.set_option("cv_wnewton_moments", value)
    assert sa.get_option("cv_wnewton_moments") == 0


def two_step_reference(shape):
    """per training set the float64 restatement of the job stopped after two Newton steps: (a0, beta, info)"""
    n, p, G, train_on = shape
    x, y = tn.problem(n, p, False, seed=2)
    foldid = cr.equal_folds(n, G, seed=2)
    moments = cr.pooled_moments(x, foldid, train_on)
    kw = {k: v for k, v in TWO_STEP.items() if k not in ("mix", "lam")}
    return x, y, foldid, [cr.pooled_job_path(x, y, T, moments[j], TWO_STEP["lam"], TWO_STEP["mix"], **kw)
                          for j, T in enumerate(cr.training_sets(foldid, train_on))]


@pytest.mark.parametrize("shape", TWO_STEP_SHAPES)
def test_two_step_inner_solves_converge_and_the_second_step_moves(shape):
    for a0, beta, info in two_step_reference(shape)[3]:
        assert info["steps"] == [2] and info["halvings"] == 0 and info["sweeps"][0] < wr.MAX_SWEEPS, info
        assert np.count_nonzero(beta) == shape[1]                  # ridge: every coordinate moves
