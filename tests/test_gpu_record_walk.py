"""The packed sample records' one walker (batched_device.hpp: row_for_each) under each of its uses, on rows of every
length from 0 to 90 entries: whatever capacity the packer gives the main record, that covers every first slot a
gather form starts its walk at (entries 0, 16, 32 and 128), every boundary of the main record, and one to four chained
overflow records of 20 entries.  The special rows are drawn at the start of every epoch (full batches) and at its
end (the tail batch).  Each case runs two batched epochs against the CPU oracle's
restatement of the same batches, to the suite's batched tolerance (test_gpu_parity: sums in hardware order, 1e-9),
and asks the solver which gather form ran.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from test_gpu_parity import STATE, TOL_BATCHED, relerr, run_both, sa  # noqa: F401  (sa: the module's fixture)

pytestmark = pytest.mark.gpu

LONGEST = 90
FORM_GLOBAL, FORM_LDS, FORM_BINNED = 0, 1, 2


def walk_problem(family, K, n, p, seed):
    """p x n sparse x, sample-major: 91 samples picked at random (`special`) have 0..90 entries, the others 3..5;
    a planted response."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(3, 6, size=n)
    special = rng.permutation(n)[:LONGEST + 1]
    lens[special] = np.arange(LONGEST + 1)
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(p, int(z), replace=False)) for z in lens]).astype(np.int32)
    val = rng.standard_normal(idx.size)
    x = sp.csc_matrix((val, idx, ptr), shape=(p, n))
    lp = (x.T @ rng.standard_normal((p, K))).T                      # K x n
    if family == "binomial":
        y = (rng.random(n) < 1.0 / (1.0 + np.exp(-lp[0]))).astype(float)
    else:
        y = np.argmax(lp + rng.gumbel(size=lp.shape), axis=0).astype(float)
    return x, np.asfortranarray(y.reshape(1, n)), special


def walk_stream(oracle, n, epochs, special, seed):
    """Uniform draws with the special rows written over the first and the last draws of every epoch (the longest
    rows last: inside the tail batch whatever its size)."""
    stream = np.array(oracle.Rng(seed).stream(n, n * epochs), copy=True)
    for e in range(epochs):
        stream[e * n:e * n + special.size] = special[::-1] if e & 1 else special
        stream[(e + 1) * n - special.size:(e + 1) * n] = special
    return stream


# family, K, penalty, n, p, batch, the form the full batches must run in.  plan_batch: the LDS form once
# batch x mean row length >= 48 K p (p >= 91 for a row of 90, so ten classes need 11 000 draws of ~4.3 entries); the
# binned form for tables beyond 80 KiB at batches of 4096 and more, and for more than 16 classes.
CASES = [
    pytest.param("binomial", 1, "elasticnet", 5000, 200, 64, FORM_GLOBAL, id="k1-global"),
    pytest.param("multinomial", 3, "elasticnet", 5000, 96, 4096, FORM_LDS, id="k3-lds"),
    pytest.param("multinomial", 10, "ridge", 14000, 92, 11000, FORM_LDS, id="k10-lds-classlane"),
    pytest.param("multinomial", 10, "elasticnet", 5000, 3000, 4096, FORM_BINNED, id="k10-binned-16"),
    pytest.param("multinomial", 20, "elasticnet", 5000, 300, 1024, FORM_BINNED, id="k20-binned-wave"),
]


@pytest.mark.parametrize("family,K,penalty,n,p,batch,form", CASES)
def test_record_walk_matches_batched_oracle(sa, oracle, family, K, penalty, n, p, batch, form):  # noqa: F811
    epochs = 2
    x, y, special = walk_problem(family, K, n, p, seed=21)
    assert n % batch >= 8                                            # there is a tail batch
    stream = walk_stream(oracle, n, epochs, special, seed=4)
    a, b = (1e-3, 0.0) if penalty == "ridge" else (1e-3, 2e-3)
    ref, got = run_both(sa, oracle, x, y, family=family, K=K, penalty=penalty, gamma=0.004, alpha=a, beta=b,
                        epochs=epochs, mode="batched", batch=batch, stream=stream)
    assert got[0] == ref[0]
    errs = {name: relerr(got[2][name], ref[2][name]) for name in STATE}
    print(family, K, batch, errs)
    for name in STATE:
        assert errs[name] < TOL_BATCHED, name
    S = sa.SagaSolver(x, y, family=family, n_classes=K)
    S.set_penalty(penalty, 0.004, a, b)
    S.upload_stream(stream[:n])
    S.run(mode="batched", batch=batch, max_epochs=1, tol=0.0)
    assert S._L.sgdnet_solver_gather_form(S._h, batch) == form       # the intended kernels are what ran
    S.close()
