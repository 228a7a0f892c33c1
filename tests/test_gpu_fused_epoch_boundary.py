"""What happens between two fused epoch launches (solver_rng.cpp, solver_epoch.cpp, batched_shards.hip).

In steady state the launch of epoch e reads the slot that the launch of epoch e - 1 filled and fills the other one, so
nothing but the kernel is enqueued: no wait for the slot's `ready` event, no record of its `freed` event (the record
is owed and made when the side stream next touches the slot).  The kernel requests round 0's cold inputs before the
start barrier's wait and the last workgroup out resets the counters with one wavefront.  None of this may change a
draw or a bit of the state, whatever is enqueued between the launches.

The path is the one bench.py drives: rng_open / rng_next / enqueue_epochs / rng_done.  Shape of
test_fit_with_the_generators_inside_the_epoch_kernel: n = 240 000, p = 100, 8 shards, 8 generators.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("w", "intercept", "g_sum", "g_sum_intercept", "g_memory")
N, P, V, GENS, SEED, EPOCHS = 240_000, 100, 8, 8, 5, 6
TOL = 1e-11                                      # as test_gpu_fused.py: the forms differ in the order of LDS additions only


@pytest.fixture(scope="module")
def sa():
    import sgdnet_amd
    sgdnet_amd.load()
    return sgdnet_amd


def relerr(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


_cache = {}


def _problem():
    if "xy" not in _cache:
        from sgdnet_amd import data as D
        pr = D.make_sparse_glm(N, P, 0.05, family="binomial", seed=23)
        _cache["xy"] = (D.as_scipy(pr), pr["y"])
    return _cache["xy"]


def _batch(dps):
    """about a quarter of a shard's epoch, a workgroup's share no multiple of the 32-draw ticket, the last round a tail"""
    b = dps // 4 - 499
    while dps % b == 0 or any((-(-b // s)) % 32 == 0 for s in (31, 32)):
        b += 1
    return b


def _host_epochs(seed, epochs):
    """R's stream as the pipeline lays it out, epoch after epoch: shard after shard, N // V draws each from the shard's
    own sample range"""
    key = ("host", seed, epochs)
    if key not in _cache:
        import sgdnet_amd as sa
        from sgdnet_amd.parallel import shard_bounds
        rng = sa.RRng(seed)
        out = []
        for _ in range(epochs):
            u = rng.unif(N)
            e = np.floor(N * u)
            dps = N // V
            for q in range(V):
                lo, hi = shard_bounds(N, V, q)
                e[q * dps:(q + 1) * dps] = lo + np.floor((hi - lo) * u[q * dps:(q + 1) * dps])
            out.append(e.astype(np.uint32))
        _cache[key] = out
    return _cache[key]


def _open(sa, seed=SEED):
    x, y = _problem()
    S = sa.SagaSolver(x, y, family="binomial", n_classes=1)
    S.set_penalty("elasticnet", 0.004, 1e-4, 1e-4)
    S.set_virtual_shards(V)
    S.rng_open(sa.RRng(seed), S.n, GENS)
    return S


def _epoch(S, batch, between=None):
    off = S.rng_next()
    if between:
        between(off)
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


def _run(sa, fused, epochs=EPOCHS, seed=SEED, after=None):
    """`epochs` epochs; after(S, e, off) runs behind epoch e's rng_done"""
    with sa.option("fused_epoch", fused):
        S = _open(sa, seed)
        batch = _batch(S.n // V)
        form = S._L.sgdnet_solver_gather_form(S._h, batch)
        for e in range(epochs):
            off = _epoch(S, batch)
            if after:
                after(S, e, off)
        return _close(S), form


def _reference(sa, seed=SEED, epochs=EPOCHS):
    """the same epochs as separate launches over converted draws (once per seed)"""
    key = ("sep", seed, epochs)
    if key not in _cache:
        st, form = _run(sa, 0, epochs, seed)
        assert form == 1
        _cache[key] = st
    return _cache[key]


def _same(got, ref, what):
    for k in STATE:
        err = relerr(got[k], ref[k])
        print(f"{what} {k}: rel {err:.3e}")
        assert err < TOL, (what, k)


def test_back_to_back_equals_synchronised_equals_separate_launches(sa):
    """(a) six epochs with one synchronisation at the end; the same six with one after each, every consumed slot read
    back; both against the separate launches.  Both slots of the first are read back at the end: the last epoch's
    draws and the generation its launch produced."""
    host = _host_epochs(SEED, EPOCHS + 1)
    sep = _reference(sa)
    tail = {}

    def read_both(S, e, off):
        if e == EPOCHS - 1:
            tail["last"] = S.get_stream(off, N)
            tail["next"] = S.get_stream(N - off, N)

    b2b, form = _run(sa, 1, after=read_both)
    assert form == 3                                  # the fused kernel really ran
    assert np.array_equal(tail["last"], host[EPOCHS - 1])
    assert np.array_equal(tail["next"], host[EPOCHS])

    def sync_and_read(S, e, off):
        S.sync()
        assert np.array_equal(S.get_stream(off, N), host[e]), e

    synced, form = _run(sa, 1, after=sync_and_read)
    assert form == 3
    _same(b2b, sep, "back to back vs separate")
    _same(synced, sep, "synchronised vs separate")
    _same(b2b, synced, "back to back vs synchronised")


def test_a_read_of_the_stream_between_fused_launches_changes_nothing(sa):
    """(b) get_stream in the middle: of the slot just consumed (behind rng_done) and of the slot about to be read
    (between rng_next and the launch, which then reads draws and is bracketed by the events again)."""
    host = _host_epochs(SEED, EPOCHS + 1)
    sep = _reference(sa)
    with sa.option("fused_epoch", 1):
        S = _open(sa)
        batch = _batch(S.n // V)
        assert S._L.sgdnet_solver_gather_form(S._h, batch) == 3
        for e in range(EPOCHS):
            seen = {}
            off = _epoch(S, batch, between=(lambda o: seen.update(ahead=S.get_stream(o, N))) if e == 3 else None)
            if e == 3:
                assert np.array_equal(seen["ahead"], host[e])
            if e == 2:
                assert np.array_equal(S.get_stream(off, N), host[e])
        st = _close(S)
    _same(st, sep, "get_stream in the middle")


def test_a_separate_launch_epoch_between_fused_launches_uses_the_side_stream(sa):
    """(b, the side stream proper) epochs 0-2 fused, epoch 3 as separate launches -- its rng_next generates on the side
    stream, into a slot whose `freed` record the fused launches left owed --, epochs 4-5 fused again."""
    host = _host_epochs(SEED, EPOCHS + 1)
    sep = _reference(sa)
    with sa.option("fused_epoch", 1):
        S = _open(sa)
        batch = _batch(S.n // V)
        for e in range(EPOCHS):
            with sa.option("fused_epoch", 0 if e == 3 else 1):
                assert S._L.sgdnet_solver_gather_form(S._h, batch) == (1 if e == 3 else 3)
                off = _epoch(S, batch)
            if e >= 3:
                assert np.array_equal(S.get_stream(off, N), host[e]), e
        st = _close(S)
    _same(st, sep, "separate launches in the middle")


def test_epoch_timing_returns_one_interval_per_launch(sa):
    """(c) five launches, five intervals -- twice: the second region reuses the first one's events"""
    with sa.option("fused_epoch", 1):
        S = _open(sa)
        batch = _batch(S.n // V)
        _epoch(S, batch)
        S.sync()
        for _ in range(2):
            S.epoch_timing(True)
            for _ in range(5):
                _epoch(S, batch)
            S.sync()
            ms, launches = S.epoch_timing(False)
            print(f"epoch_timing: {launches} launches, {ms:.3f} ms")
            assert launches == 5
            assert 0.0 < ms < 5 * 50.0                # (an epoch here takes well under a millisecond)
        _epoch(S, batch)                              # not timed
        S.sync()
        assert S.epoch_timing(False) == (0.0, 0)
        _close(S)


def test_two_solvers_alternating_on_one_device_share_nothing(sa):
    """(d) two solvers with different seeds take turns (a fused epoch holds every CU, so each turn ends with a
    synchronisation); each must end where it ends alone, and each counts its own timed launches."""
    epochs = 4
    seeds = (SEED, SEED + 6)
    refs = [_reference(sa, s, epochs) for s in seeds]
    host = [_host_epochs(s, epochs) for s in seeds]
    with sa.option("fused_epoch", 1):
        solvers = [_open(sa, s) for s in seeds]
        batch = _batch(N // V)
        for S in solvers:
            S.epoch_timing(True)
        offs = [0, 0]
        for e in range(epochs):
            for i, S in enumerate(solvers):
                if i == 1 and e == epochs - 1:
                    break                              # (the second solver: one launch fewer inside its timed region)
                offs[i] = _epoch(S, batch)
                S.sync()
        counts = [S.epoch_timing(False)[1] for S in solvers]
        assert counts == [epochs, epochs - 1]
        offs[1] = _epoch(solvers[1], batch)
        for i, S in enumerate(solvers):
            assert np.array_equal(S.get_stream(offs[i], N), host[i][epochs - 1]), i
        states = [_close(S) for S in solvers]
    for i in range(2):
        _same(states[i], refs[i], f"solver {i} beside the other")
