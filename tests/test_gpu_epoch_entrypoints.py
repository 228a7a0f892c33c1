"""The three entry points that run batched epochs -- sgdnet_solver_run, _enqueue_epochs and _profile_epoch
(solver_epoch.cpp) -- start in one prologue, begin_batched_epochs, and run the same launches.  What that prologue
carries from one call to the next (stream_base, stream_wrap, batch_seq, the slots' raw flags, the upload it may skip)
is checked by mixing the entry points over consecutive epochs of one stream: the state must be that of one plain run.

profile_epoch is what bench.py reads `roofline.achieved` and `kernel_alone` from; its launch counts are asserted too,
because they come out of the same event bookkeeping as the launches.

The bound is the one test_gpu_fused.py holds between two launch structures that sum in different orders; the entry
points run the same launches, so they sit inside it (run-to-run differences <= 1.5e-13).
"""
import numpy as np
import pytest

import test_gpu_fused_raw_stream as raw

pytestmark = pytest.mark.gpu

STATE = ("w", "intercept", "g_sum", "g_sum_intercept", "g_memory")
EPOCHS = 3
BOUND = 1e-11


@pytest.fixture(scope="module")
def sa():
    import sgdnet_amd
    sgdnet_amd.load()
    return sgdnet_amd


def relerr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


def _sparse(family, K, n, p, seed):
    from sgdnet_amd import data as D
    pr = D.make_sparse_glm(n, p, 0.08, family=family, n_classes=K, seed=seed)
    return D.as_scipy(pr), pr["y"]


def _dense_gaussian(n, p, seed):
    rng = np.random.default_rng(seed)
    x = np.asfortranarray(rng.standard_normal((p, n)))
    y = rng.standard_normal(p) @ x + 0.1 * rng.standard_normal(n)
    return x, np.asfortranarray(y.reshape(1, n))


# name: (problem, family, K, centred, V, fused_epoch, batch, expected gather form or None)
CASES = {
    # compact-record LDS form, a tail batch of 200, the gradient memory moves into the records (m_to_record)
    "sparse-binomial": (lambda: _sparse("binomial", 1, 3000, 64, 5), "binomial", 1, False, 0, 1, 700, None),
    # ... with implicit centring: launch_cw_init
    "sparse-binomial-centred": (lambda: _sparse("binomial", 1, 3000, 64, 5), "binomial", 1, True, 0, 1, 700, None),
    # enqueue_epoch_kernels_vs: separate launches with merges
    "shards-separate": (lambda: _sparse("gaussian", 1, 20_000, 50, 5), "gaussian", 1, True, 2, 0, 900, 1),
    # the plain fused launch outside the graph
    "shards-fused": (lambda: _sparse("gaussian", 1, 20_000, 50, 5), "gaussian", 1, True, 2, 1, 900, 3),
    # dense gather, no records
    "dense-gaussian": (lambda: _dense_gaussian(2000, 40, 11), "gaussian", 1, False, 0, 1, 300, None),
    # the K > 1 form: the gradient memory stays in its array
    "sparse-multinomial": (lambda: _sparse("multinomial", 3, 3000, 64, 7), "multinomial", 3, False, 0, 1, 700, None),
}

RUN, ENQ, PROF = "run", "enqueue", "profile"
ORDERS = [(ENQ, PROF, RUN), (PROF, RUN, ENQ)]


def _solver(sa, x, y, family, K, c, V):
    S = sa.SagaSolver(x, y, family=family, n_classes=K, x_center_scaled=c)
    S.set_penalty("elasticnet", 0.004, 1e-4, 1e-4)
    if V:
        S.set_virtual_shards(V)
        S.upload_stream(S.sharded_stream([sa.RRng(70 + v) for v in range(V)], EPOCHS))
        return S, V * (S.n // V)
    S.upload_stream(sa.RRng(5).stream(S.n, EPOCHS * S.n))
    return S, S.n


def _state(S, V):
    S.sync()
    st = {k: S.get(k) for k in STATE}
    if V:
        S.set_virtual_shards(0)
    S.close()
    return st


@pytest.mark.parametrize("case", list(CASES))
def test_mixed_entry_points_leave_the_state_of_one_run(sa, case):
    make, family, K, centred, V, fused, batch, form = CASES[case]
    x, y = make()
    c = np.random.default_rng(9).normal(0.05, 0.1, x.shape[0]) if centred else None
    with sa.option("fused_epoch", fused):
        S, draws = _solver(sa, x, y, family, K, c, V)
        got_form = S._L.sgdnet_solver_gather_form(S._h, batch)
        print(f"{case}: gather form {got_form}")
        if form is not None:
            assert got_form == form
        ep, _ = S.run(mode="batched", batch=batch, draws_per_epoch=draws, max_epochs=EPOCHS, tol=0.0)
        assert ep == EPOCHS
        want = _state(S, V)
        per_launch = draws // V if V else draws
        launches = 1 if got_form == 3 else -(-per_launch // batch)
        for order in ORDERS:
            S, draws = _solver(sa, x, y, family, K, c, V)
            for e, how in enumerate(order):
                kw = dict(batch=batch, stream_offset=e * draws, draws_per_epoch=draws)
                if how == RUN:
                    ep, _ = S.run(mode="batched", max_epochs=1, tol=0.0, **kw)
                    assert ep == 1
                elif how == ENQ:
                    S.enqueue_epochs(1, **kw)
                else:
                    prof = S.profile_epoch(**kw)
                    print(f"{case} {'/'.join(order)}: profile_epoch reports {prof['gather_launches']} gather and "
                          f"{prof['sweep_launches']} sweep launches, expected {launches}")
                    assert prof["gather_launches"] == prof["sweep_launches"] == launches
            got = _state(S, V)
            for k in STATE:
                err = relerr(got[k], want[k])
                print(f"{case} {'/'.join(order)} {k}: rel {err:.3e}")
                assert err < BOUND, (order, k)


def test_run_and_enqueue_epochs_agree_through_the_sample_order_pipeline(sa):
    """The fused form fed by the sample-order pipeline with several generators (the helpers and the problem of
    test_gpu_fused_raw_stream.py), three epochs, driven once through enqueue_epochs and once through run: the same
    state, the same words in both slots of the stream buffer, and R's generator left in the same place."""
    n = 240_000
    x, y = raw._problem(n)
    out = {}
    with sa.option("fused_epoch", 1):
        for how in (ENQ, RUN):
            S, rng = raw._open(sa, x, y)
            batch = raw._batch(S.n // raw.V)
            assert S._L.sgdnet_solver_gather_form(S._h, batch) == 3
            for _ in range(EPOCHS):
                if how == ENQ:
                    raw._epoch(S, batch)
                else:
                    off = S.rng_next()
                    ep, _ = S.run(mode="batched", batch=batch, stream_offset=off, draws_per_epoch=S.n, max_epochs=1,
                                  tol=0.0)
                    assert ep == 1
                    S.rng_done()
            S.sync()
            slots = [S.get_stream(q * n, n) for q in range(2)]
            out[how] = (raw._close(S), slots, rng.unif(32))
    (st_e, slots_e, next_e), (st_r, slots_r, next_r) = out[ENQ], out[RUN]
    for k in STATE:
        err = relerr(st_r[k], st_e[k])
        print(f"pipeline run vs enqueue_epochs {k}: rel {err:.3e}")
        assert err < BOUND, k
    for q in range(2):
        assert np.array_equal(slots_e[q], slots_r[q]), q
    assert np.array_equal(next_e, next_r)
