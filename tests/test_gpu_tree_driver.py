"""What the tree step driver (csrc/tree_driver.hip) hands to its walks, seen from outside: a walk that is steered by an argument
— the order of accel_tree's targets, the tracers' walk without timer, statistics and back-off — leaves the context's own
settings as they were.  Needs an MI355X."""
import numpy as np
import pytest

from tests import _routes as routes

pytestmark = pytest.mark.gpu
DT = 0.1


# BVH, leaves of 64: 4097 bodies take the one-pass walk, 300 the fused one; the quad tree walks its leaves' copies
@pytest.mark.parametrize("kind,n", [("bvh", 4097), ("bvh", 300), ("quad", 300)])
def test_accel_tree_at_the_bodies_ignores_the_order_and_leaves_it_alone(nb, monkeypatch, capfd, kind, n):
    C = nb._capi
    tree = C.TREE_BVH if kind == "bvh" else C.TREE_QUAD
    pos, vel, w = nb.scenes.plummer(n, seed=0x0ACC + n)
    monkeypatch.setenv("NBODY_TRACE", "1")
    got = {}
    with C.Context(0) as c:
        for order in (C.ORDER_AS_WRITTEN, C.ORDER_CONSISTENT):
            c.set_params(theta=50.0, leaf_size=64, order=order)
            c.upload(pos, vel, w)
            capfd.readouterr()
            got[order] = c.accel_tree(tree)
            ran = routes.parse(capfd.readouterr().err)
            assert c.get_params().order == order
            assert len(ran) == 1 and ran[0].n_tgt == n
            if kind == "bvh":
                assert ran[0].route == routes.expected_bvh_route(n, 64, 1, lab=False)
    a, b = got[C.ORDER_AS_WRITTEN], got[C.ORDER_CONSISTENT]
    assert a.shape == (n, 2) and np.isfinite(a).all() and np.abs(a).max() > 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_tracers_walk_leaves_timer_statistics_and_back_off_to_the_bodies(nb, orc, monkeypatch, capfd):
    """Three BVH steps with five tracers, a Timer and the walk statistics on; then the tracers go, the statistics are switched off
    and three more steps follow.  Each of the first three leaves the statistics and the Timer's launch count of the same step
    without tracers; of the later three the first is plain (the walks with statistics left no history to estimate from) and the
    other two stand as steps enqueued ahead — which a context whose statistics switch or back-off the tracers' walk had moved
    would not take; the bodies are the oracle's after all six."""
    C = nb._capi
    n = 4097
    pos, vel, w = nb.scenes.plummer(n, seed=0x7AC3)
    rng = np.random.default_rng(5)
    tp, tv = pos[rng.choice(n, 5, replace=False)] + np.float32(0.01), rng.normal(0, 1, (5, 2)).astype(np.float32)
    monkeypatch.setenv("NBODY_TRACE", "1")
    seen = {}
    for tracers in (True, False):
        with C.Context(0) as c:
            c.set_params(theta=50.0, leaf_size=64, order=C.ORDER_AS_WRITTEN)
            c.upload(pos, vel, w)
            if tracers:
                c.upload_tracers(tp, tv)
            t = C.Timer()
            try:
                c.set_timer(t)
                c.walk_stats(True)
                stats, launches = [], []
                for _ in range(3):
                    c.update_tree(C.TREE_BVH, DT, 1)
                    stats.append(c.walk_stats(True))
                    launches.append(t.read()[1])
                c.walk_stats(False)
                if tracers:
                    assert c.n_tracers == 5
                    c.upload_tracers(np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))
                capfd.readouterr()
                c.update_tree(C.TREE_BVH, DT, 3)
                err = capfd.readouterr().err
            finally:
                c.set_timer(None)
                t.close()
            seen[tracers] = (stats, launches, err, c.download())
    stats, launches, err, got = seen[True]
    assert all(s[0] > 0 for s in stats), stats
    assert stats == seen[False][0] and launches == seen[False][1], (stats, seen[False][0], launches, seen[False][1])
    ran = routes.parse(err)
    assert [(r.route, r.ahead, r.n_tgt) for r in ran] == [(routes.TILE, 0, n), (routes.TILE, 1, n), (routes.TILE, 1, n)], [tuple(r) for r in ran]
    assert err.count("step ahead: build verdict 1") == 2 and "step ahead: build verdict 0" not in err, err[-1200:]
    rp, rv, rw, rids, _ = orc.update_bvh(pos, vel, w, delta=DT, theta=50.0, leaf_size=64, mode=orc.AS_WRITTEN, nsteps=6, nthreads=16)
    for g in (got, seen[False][3]):
        assert np.array_equal(g[3], rids) and np.array_equal(g[2], rw) and np.array_equal(g[0], rp) and np.array_equal(g[1], rv)
