"""The stages of one fit of the covariance family (sgdnet_amd/csrc/covariance.hip: covariance_run, wcovariance_run,
mcovariance_run, wmcovariance_run) one by one, through sgdnet_covariance_probe, against exact references
(tests/covariance_passes_reference.py; tests/test_gpu_cv_covariance_passes.py does the same for the cross-validations and says why).

  bounded   the means (exactly 0 without centring; sparse: over all n rows), the response sums, and every DEFINED entry of M:
            dense about the returned centres, sparse over the terms of the kernel's four-term identity (the response block
            of a sparse fit's M is documented as undefined and is the only thing left out; the reference says which it is)
  bitwise   M == M'; the scale stage in full from the returned M -- the narrow path kernels' c, the wide S from the upper
            triangle in the kernel's order of operations, its pad exactly 0, ld, diag S, c~ (wide_scale_kernel as
            covariance.hip instantiates it, cov_wide_group_scale_kernel); descending rows against ascending; a second call
The wide feature limit (4531) is not here: its matrix is 164 MB and its long-double truth takes minutes.  Each check prints
the value closest to its bound (run with -s)."""
import numpy as np
import pytest

import covariance_passes_reference as R

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def probe():
    import torch  # noqa: F401  -- before libsgdnet_hip.so (sgdnet_amd/_lib.py)
    import sgdnet_amd
    L = sgdnet_amd.load()
    if L.sgdnet_device_count() < 1:
        pytest.fail("GPU tests need a HIP device; the backend has no CPU fallback")
    assert L.sgdnet_covariance_max_features() == R.COV_MAX_FEATURES and L.sgdnet_mcovariance_max_features(3) == R.mcov_max_features(3)
    from sgdnet_amd import diagnostics
    return diagnostics


def run(probe, case):
    return probe.covariance_probe(case.x, case.y, case.scale, float(case.mixes[0]), case.lam[0], wide=case.wide, multi=case.multi,
                                  centre=case.centre)


@pytest.mark.parametrize("name", list(R.SINGLE_DENSE))
def test_dense(probe, name):
    case = R.single_dense_case(name)
    R.check_single(run(probe, case), case)


def test_dense_uncentred(probe):
    case = R.single_dense_case("n65_P31", centre=False)
    R.check_single(run(probe, case), case)


@pytest.mark.parametrize("n,K,wide,centre", [(600, 0, False, True), (600, 3, True, True), (257, 0, False, False), (257, 2, False, True),
                                             (1, 0, False, True), (255, 0, True, True)])
def test_sparse(probe, n, K, wide, centre):
    case = R.single_sparse_case(n, K=K, wide=wide, centre=centre)
    R.check_single(run(probe, case), case)


@pytest.mark.parametrize("n,K", [(600, 0), (257, 2)])
def test_descending_rows_give_the_bits_of_ascending_rows(probe, n, K):
    a, d = run(probe, R.single_sparse_case(n, K=K)), run(probe, R.single_sparse_case(n, K=K, descending=True))
    p = 11
    d.M[p:, p:] = a.M[p:, p:] = 0.0                 # the response block of a sparse fit's M is not defined
    R.same_bits(d, a, f"sparse {n}")


def test_a_matrix_that_stores_nothing(probe):
    case = R.empty_sparse_single_case()
    o = run(probe, case)
    R.check_single(o, case)
    assert np.all(o.M[:case.p, :] == 0.0) and np.all(o.c == 0.0)


@pytest.mark.parametrize("name", ["n257_P33_K17", "w65x209_K2"])
def test_a_second_call_returns_the_same_bits(probe, name):
    case = R.single_dense_case(name)
    R.same_bits(run(probe, case), run(probe, case), name)


def test_the_probe_refuses_what_the_plan_refuses(probe):
    """the feature limits in the plan's words and with its code; the fit's own refusal of the same shape says the same"""
    import sgdnet_amd as sa
    from sgdnet_amd import SgdnetError
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal((20, R.COV_MAX_FEATURES + 1)), rng.standard_normal(20)
    needle = "mode = covariance needs no more features than sgdnet_covariance_max_features()"
    with pytest.raises(SgdnetError) as e:
        probe.covariance_probe(x, y, np.ones(x.shape[1]), 0.5, [0.1])
    assert e.value.code == EUNSUPPORTED and needle in str(e.value) and "199 features (limit 198)" in str(e.value)
    with pytest.raises(SgdnetError) as e:
        sa.sgdnet(x, y, alpha=0.5, lambda_=[0.1], mode="covariance")
    assert e.value.code == EUNSUPPORTED and needle in str(e.value)
    assert probe.covariance_probe(x, y, np.ones(x.shape[1]), 0.5, [0.1], wide=True).ld == 208
    Y = rng.standard_normal((20, 3))
    needle = "mode = mcovariance needs no more features than sgdnet_mcovariance_max_features(n_classes)"
    with pytest.raises(SgdnetError) as e:
        probe.covariance_probe(x[:, :R.mcov_max_features(3) + 1], Y, np.ones(R.mcov_max_features(3) + 1), 0.5, [0.1])
    assert e.value.code == EUNSUPPORTED and needle in str(e.value)
    with pytest.raises(SgdnetError) as e:
        sa.sgdnet_mcovariance(x[:, :R.mcov_max_features(3) + 1], Y, alpha=0.5, lambda_=[0.1])
    assert e.value.code == EUNSUPPORTED and needle in str(e.value)
    with pytest.raises(SgdnetError) as e:
        probe.covariance_probe(x[:, :5], Y, np.ones(5), 0.5, [0.1], multi=False)
    assert e.value.code == EINVAL and "sgdnet_covariance_probe: invalid argument" in str(e.value)
    with pytest.raises(SgdnetError) as e:
        probe.covariance_probe(x[:, :5], y, np.ones(5), 1.5, [0.1])
    assert e.value.code == EINVAL
