"""The f32 BVH step enqueued ahead of the host (tree_driver.hip, bvh_step_ahead) at the sizes where its preparation changes
shape, against the oracle bit for bit — and, because the plain sequence gives the same bits, with the trace saying how many
steps stood as step-ahead and which preparation they used (tests/_routes.py).  Needs an MI355X.

Product library: the single-pass scan (walk_scan_est_tail), work-groups of 1 024 targets.  Laboratory library with
NBODY_WALK_FUSED_SCAN_MAX=0: the path the product takes above 2^24 bodies — the library scan plus walk_check_est_tail with
clamp(n / 2048, 32, 128) work-groups, and the phases timed by events instead of the kernels' clock."""
import numpy as np
import pytest

from tests import _routes as routes

pytestmark = pytest.mark.gpu
F32 = np.float32
_GALAXY_N = 151405


def _scene(nb, name, n):
    if name == "plummer":
        return nb.scenes.plummer(n, seed=0x5EED0400 + n % 97)
    pos, vel, w = nb.scenes.galaxy()
    sel = np.random.default_rng(n).choice(pos.shape[0], n, replace=False)
    sel.sort()
    sel[:2] = (0, 1)                                       # keep the two heavy bodies
    return pos[sel].copy(), vel[sel].copy(), w[sel].copy()


def _run(nb, orc, capfd, scene, n, order_name, first, prep):
    """`first` steps in one call, one more in a second: the first step of a context is plain (no walk to estimate from), every
    later one must stand as a step enqueued ahead with the preparation `prep`.  Returns (Counting, rows)."""
    C = nb._capi
    order = C.ORDER_AS_WRITTEN if order_name == "as_written" else C.ORDER_CONSISTENT
    pos, vel, w = _scene(nb, scene, n)
    capfd.readouterr()
    with C.Context(0) as c:
        c.set_params(theta=50.0, leaf_size=64, order=order)
        c.upload(pos, vel, w)
        cnt = C.Counting()
        c.update_tree(C.TREE_BVH, 0.1, first, cnt)
        c.update_tree(C.TREE_BVH, 0.1, 1, cnt)
        got = c.download()
    err = capfd.readouterr().err
    mode = orc.AS_WRITTEN if order_name == "as_written" else orc.CONSISTENT
    rp, rv, rw, rids, _ = orc.update_bvh(pos, vel, w, delta=0.1, theta=50.0, leaf_size=64, mode=mode, nsteps=first + 1, nthreads=16)
    assert np.array_equal(got[3], rids) and np.array_equal(got[2], rw)
    assert np.array_equal(got[0], rp) and np.array_equal(got[1], rv)
    ran = routes.parse(err)
    assert err.count("step ahead: build verdict 1") == first and "step ahead: build verdict 0" not in err, err[-1200:]
    assert [r.prep for r in ran if r.ahead] == [prep] * first, [tuple(r) for r in ran]
    assert [(r.route, r.prep, r.n_tgt) for r in ran if not r.ahead] == [(routes.TILE, "plain", n)], [tuple(r) for r in ran]
    assert all(r.route == routes.TILE and r.n_tgt == n and r.arm == "exact" for r in ran)
    assert cnt.build_bvh > 0 and cnt.sum_gravity > 0 and cnt.post_calculations > 0
    return cnt, got


# 4096: the smallest step ahead, exactly four work-groups; 4097: a fifth holding one target; 5121; 66 * 1024 + 1: 67 groups, the
# last of which looks back past 64 predecessors
@pytest.mark.parametrize("order_name", ["as_written", "consistent"])
@pytest.mark.parametrize("scene", ["plummer", "galaxy"])
@pytest.mark.parametrize("n", [4096, 4097, 5121, 66 * 1024 + 1])
def test_step_ahead_with_the_fused_scan_at_its_edge_sizes(nb, orc, monkeypatch, capfd, n, scene, order_name):
    monkeypatch.setenv("NBODY_TRACE", "1")
    _run(nb, orc, capfd, scene, n, order_name, 4, "scan-tail")


# 4096, 4097: 32 work-groups, most threads idle; 70 001: 34; 262 147: the cap of 128, every thread loops (the galaxy scene has
# 151 405 bodies, so that size is Plummer only)
@pytest.mark.parametrize("order_name", ["as_written", "consistent"])
@pytest.mark.parametrize("scene,n", [("plummer", 4096), ("galaxy", 4096), ("plummer", 4097), ("galaxy", 4097), ("plummer", 70001),
                                     ("galaxy", 70001), ("plummer", 262147)])
def test_step_ahead_with_the_three_kernel_tail(nb, orc, lab, monkeypatch, capfd, scene, n, order_name):
    assert n <= _GALAXY_N or scene == "plummer"
    monkeypatch.setenv("NBODY_TRACE", "1")
    monkeypatch.setenv("NBODY_WALK_FUSED_SCAN_MAX", "0")
    _run(nb, orc, capfd, scene, n, order_name, 4 if n < 70000 else 2, "check-tail")


def test_three_kernel_tail_times_the_phases_the_stamps_time(nb, lab, monkeypatch, capfd):
    """The three-kernel tail's steps are timed by events, the fused scan's by the kernels' clock: the same phases.  Sense and
    margin are those of test_phase_stamps_and_event_records_time_the_same_phases (tests/test_gpu_tree.py): build and walk
    within 15 % of the event-timed figures, the last phase not above 1.5 x + 1 ms of them."""
    C = nb._capi
    pos, vel, w = nb.scenes.galaxy()
    out = {}
    for name, cap in (("stamps", None), ("events", "0")):
        if cap is not None:
            monkeypatch.setenv("NBODY_WALK_FUSED_SCAN_MAX", cap)
        with C.Context(0) as c:
            c.upload(pos, vel, w)
            monkeypatch.setenv("NBODY_TRACE", "1")                   # which preparation: from the warm-up steps' trace
            capfd.readouterr()
            c.update_tree(C.TREE_BVH, 0.1, 5)
            ran = routes.parse(capfd.readouterr().err)
            assert [r.prep for r in ran if r.ahead] == ["scan-tail" if cap is None else "check-tail"] * 4, [tuple(r) for r in ran]
            monkeypatch.setenv("NBODY_TRACE", "0")                   # ... and the timed steps print nothing
            cnt = C.Counting()
            c.update_tree(C.TREE_BVH, 0.1, 100, cnt)
            out[name] = (cnt.build_bvh, cnt.sum_gravity, cnt.post_calculations, c.download())
    a, b = out["stamps"], out["events"]
    print(f"[phases] stamps {a[:3]} events {b[:3]}")
    assert all(x > 0 for x in a[:3] + b[:3])
    assert abs(a[0] - b[0]) <= 0.15 * b[0] and abs(a[1] - b[1]) <= 0.15 * b[1], (a[:3], b[:3])
    assert a[2] <= b[2] * 1.5 + 1e-3
    assert all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))


@pytest.mark.parametrize("order_name", ["as_written", "consistent"])
def test_three_kernel_tail_flags_a_wrapped_estimate(nb, orc, lab, monkeypatch, capfd, order_name):
    """NBODY_WALK_TILE_POISON=1 fills the history with 0xFFFFFFFF before every walk that uses it: walk_check_est_tail must flag
    it (`overflow 1`, the walk kernel returns at once), the step is walked again the plain way — which meets the same history,
    flags it too and walks without an estimate (`estimate none`) — and the trajectory is still the oracle's."""
    C = nb._capi
    n = 4097
    monkeypatch.setenv("NBODY_TRACE", "1")
    monkeypatch.setenv("NBODY_WALK_FUSED_SCAN_MAX", "0")
    monkeypatch.setenv("NBODY_WALK_TILE_POISON", "1")
    order = C.ORDER_AS_WRITTEN if order_name == "as_written" else C.ORDER_CONSISTENT
    pos, vel, w = _scene(nb, "plummer", n)
    capfd.readouterr()
    with C.Context(0) as c:
        c.set_params(theta=50.0, leaf_size=64, order=order)
        c.upload(pos, vel, w)
        c.update_tree(C.TREE_BVH, 0.1, 4)
        got = c.download()
    err = capfd.readouterr().err
    ahead = [ln for ln in err.splitlines() if "tile walk (step ahead)" in ln]
    assert len(ahead) == 3 and all(ln.endswith("overflow 1") for ln in ahead), err[-1500:]
    assert err.count("step ahead: build verdict 1") == 3
    assert err.count("estimate none") == 3
    ran = routes.parse(err)
    assert [r.prep for r in ran if r.ahead] == ["check-tail"] * 3
    mode = orc.AS_WRITTEN if order_name == "as_written" else orc.CONSISTENT
    rp, rv, rw, rids, _ = orc.update_bvh(pos, vel, w, delta=0.1, theta=50.0, leaf_size=64, mode=mode, nsteps=4, nthreads=16)
    assert np.array_equal(got[3], rids) and np.array_equal(got[2], rw) and np.array_equal(got[0], rp) and np.array_equal(got[1], rv)
