"""The fused epoch kernel over a slot of the sample-order pipeline that holds the generators' RAW words
(saga_batched.hip: K1CompactT<true>): a word becomes a draw where the draw loop first needs it as a sample id, the
kernel writes nothing back, and the slot is still raw when the epoch is over.  solver.cpp keeps the record per slot
and converts a raw slot exactly once for every other reader (sgdnet_solver_get_stream, the separate launches).

The path is the one bench.py drives: rng_open / rng_next / enqueue_epochs / rng_done.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("w", "intercept", "g_sum", "g_sum_intercept", "g_memory")
V, GENS, SEED = 8, 8, 5


@pytest.fixture(scope="module")
def sa():
    import sgdnet_amd
    sgdnet_amd.load()
    return sgdnet_amd


def relerr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


_problems = {}


def _problem(n, p=100, seed=23):
    if (n, p) not in _problems:
        from sgdnet_amd import data as D
        pr = D.make_sparse_glm(n, p, 0.05, family="binomial", seed=seed)
        _problems[(n, p)] = (D.as_scipy(pr), pr["y"])
    return _problems[(n, p)]


def _batch(dps):
    """A window of about a quarter of a shard's epoch such that a workgroup's share ceil(m / S) is no multiple of the
    32-draw ticket (S = 31 with the generators' CUs set aside, 32 without) and the shard's last round is a tail."""
    b = dps // 4 - 499
    while dps % b == 0 or any((-(-b // s)) % 32 == 0 for s in (31, 32)):
        b += 1
    assert 0 < b < dps
    return b


def _open(sa, x, y, v=V):
    S = sa.SagaSolver(x, y, family="binomial", n_classes=1)
    S.set_penalty("elasticnet", 0.004, 1e-4, 1e-4)
    S.set_virtual_shards(v)
    rng = sa.RRng(SEED)
    S.rng_open(rng, S.n, GENS)
    return S, rng


def _epoch(S, batch):
    off = S.rng_next()
    S.enqueue_epochs(1, batch=batch, stream_offset=off, draws_per_epoch=S.n)
    S.rng_done()
    return off


def _close(S):
    S.sync()
    st = {k: S.get(k) for k in STATE}
    S.rng_close()
    S.set_virtual_shards(0)
    S.close()
    return st


def _run(sa, x, y, fused, epochs, v=V):
    with sa.option("fused_epoch", fused):
        S, rng = _open(sa, x, y, v)
        batch = _batch(S.n // v)
        form = S._L.sgdnet_solver_gather_form(S._h, batch)
        for _ in range(epochs):
            _epoch(S, batch)
        st = _close(S)
    return st, form, rng.unif(32)                        # (the caller's generator: where the device left R's stream)


_separate = {}


def _separate_launches(sa, n, epochs=3):
    """the reference of this file: the same epochs as separate launches over converted draws (computed once per n)"""
    if n not in _separate:
        _separate[n] = _run(sa, *_problem(n), 0, epochs)
    return _separate[n]


def _host_epoch(rng, n, v=V):
    """one epoch of R's stream as the pipeline lays it out: shard after shard, n // V draws each from the shard's own
    sample range (r_rng_device.hip convert_at); the n % V positions behind them belong to no shard"""
    from sgdnet_amd.parallel import shard_bounds
    u = rng.unif(n)
    out = np.floor(n * u)
    dps = n // v
    for q in range(v):
        lo, hi = shard_bounds(n, v, q)
        out[q * dps:(q + 1) * dps] = lo + np.floor((hi - lo) * u[q * dps:(q + 1) * dps])
    return out.astype(np.uint32)


@pytest.mark.parametrize("fused", [1, 2])
@pytest.mark.parametrize("n", [240_000, 240_003])          # the second: unequal shard sizes
def test_fused_over_raw_words_equals_separate_launches_over_draws(sa, n, fused):
    epochs = 3
    x, y = _problem(n)
    sep, form0, next0 = _separate_launches(sa, n, epochs)
    one, form1, next1 = _run(sa, x, y, fused, epochs)
    assert form1 == 3 and form0 == 1                     # the fused kernel really ran / really did not
    for k in STATE:
        err = relerr(one[k], sep[k])
        print(f"n={n} fused_epoch={fused} {k}: rel {err:.3e}")
        assert err < 1e-11, k
    host = sa.RRng(SEED)
    host.stream(n, epochs * n)
    want = host.unif(32)
    assert np.array_equal(want, next1) and np.array_equal(want, next0)


def test_a_consumed_slot_reads_back_as_draws_once(sa):
    n = 240_003
    x, y = _problem(n)
    sep, _, _ = _separate_launches(sa, n, 3)
    host = sa.RRng(SEED)
    with sa.option("fused_epoch", 1):
        S, _ = _open(sa, x, y)
        batch = _batch(S.n // V)
        assert S._L.sgdnet_solver_gather_form(S._h, batch) == 3
        off = _epoch(S, batch)                           # fused, over raw words
        want = _host_epoch(host, n)
        first = S.get_stream(off, n)
        assert np.array_equal(first, want)
        assert np.array_equal(S.get_stream(off, n), first)        # a second conversion would scramble it
        _epoch(S, batch)                                 # fused again, on the other slot
    with sa.option("fused_epoch", 0):
        assert S._L.sgdnet_solver_gather_form(S._h, batch) == 1
        _epoch(S, batch)                                 # separate launches on the slot the in-kernel generators filled
        st = _close(S)
    for k in STATE:
        err = relerr(st[k], sep[k])
        print(f"mixed fused / separate {k}: rel {err:.3e}")
        assert err < 1e-11, k


def test_the_fallback_keeps_working_through_the_pipeline(sa):
    """p = 51: the fused form refuses an odd number of features, so fused_epoch = 1 runs the separate launches; every
    one of them reads draws, whatever the pipeline left in the slot."""
    x, y = _problem(40_000, p=51, seed=6)
    one, form1, _ = _run(sa, x, y, 1, 2, v=4)
    sep, form0, _ = _run(sa, x, y, 0, 2, v=4)
    assert form1 == 1 and form0 == 1
    for k in STATE:
        err = relerr(one[k], sep[k])
        print(f"fallback {k}: rel {err:.3e}")
        assert err < 1e-11, k
