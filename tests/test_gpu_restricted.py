"""Restricted ensembles on the device (nb.RestrictedEnsemble over nbody_restricted_*): B worlds of n bodies with m tracers each.
The bodies are compared with the oracle's update_direct and with nb.Ensemble, bit for bit; the tracers of every world with the
oracle's direct_accel at them (native accumulation) + Euler in numpy, bit for bit under EXACT, within the frozen tolerance of
tests/_tol.py under FAST; AUTO with the composition of the two.  Needs an MI355X.

Sizes: n = 1, 2, 7, 65 (the bodies split their sources over lanes, the tracers never do), 129 / 257 / 300 / 1000 (one target per
lane on both sides), 4096 (48 KB of LDS); m around every multiple of a block's 256 lanes up to 8 tracers per lane."""
import numpy as np
import pytest

from _tol import check_fast
from test_gpu_ensemble import _assert_worlds_equal, _fast_worlds, _oracle_steps, _same_bits, _worlds
from test_gpu_tracers import _crossing_tracers, _euler, _outside_fast, _tracer_set

pytestmark = pytest.mark.gpu
F32 = np.float32
NTH = 16
DT = 0.1
CLAMP = 0.001


def _tracers_for(pos, m, seed, with_skip=True):
    """m tracers for every world of pos[B, n, 2] (test_gpu_tracers._tracer_set per world: points on bodies, at 0.5 sqrt(clamp)
    from bodies, random ones and — m allowing — the skip cases) -> (tp[B, m, 2], tv[B, m, 2])."""
    tps, tvs = [], []
    for k in range(pos.shape[0]):
        tp, tv, _ = _tracer_set(np.random.default_rng(seed + k), pos[k], F32, m, with_skip=with_skip)
        assert tp.shape == (m, 2)
        tps.append(tp), tvs.append(tv)
    return np.stack(tps), np.stack(tvs)


def _exact_accel(orc, pos, w, tp, clamp=CLAMP):
    """The oracle's sum at the tracers of every world: direct_accel(pos_k, w_k, target_pos=tp_k, accum="native")."""
    return np.stack([orc.direct_accel(pos[k], w[k], target_pos=tp[k], clamp=clamp, accum="native", nthreads=NTH)[0].astype(F32)
                     for k in range(pos.shape[0])])


def _exact_steps(orc, pos, vel, w, tp, tv, steps, clamp=CLAMP):
    """Both references, step by step: the tracers by direct_accel at the pre-step bodies + Euler, the bodies by update_direct."""
    for _ in range(steps):
        tp, tv = _euler(tp, tv, _exact_accel(orc, pos, w, tp, clamp), DT)
        pos, vel = _oracle_steps(orc, pos, vel, w, 1, clamp=clamp, delta=DT)
    return pos, vel, tp, tv


def _run(nb, pos, vel, w, tracers, arith, calls=(3,), **kw):
    with nb.RestrictedEnsemble(pos, vel, w, tracers, arith=arith, **kw) as r:
        for k in calls:
            r.update(DT, None, n_steps=k)
        return (*r.particles()[:2], *r.tracers())


# ------------------------------------------------------------------ 1. EXACT against two references
@pytest.mark.parametrize("n,m", [(1, 1), (2, 257), (65, 600), (257, 256), (1000, 257), (4096, 300)])
def test_exact_bodies_and_tracers_equal_the_oracle_bit_for_bit(nb, orc, n, m):
    pos, vel, w = _worlds(nb, n, 3, seed=1100 + n, awkward_at=1)
    tp, tv = _tracers_for(pos, m, 2000 + n)
    with nb.RestrictedEnsemble(pos, vel, w, (tp, tv), arith="exact") as r:
        assert r.shape == (3, n, m)
        r.update(DT, None, n_steps=3)
        p, v, w2 = r.particles()
        gp, gv = r.tracers()
    assert gp.shape == gv.shape == (3, m, 2) and gp.dtype == F32 and np.array_equal(w2, w)
    rp, rv, rtp, rtv = _exact_steps(orc, pos, vel, w, tp, tv, 3)
    _assert_worlds_equal(p, rp, "positions")
    _assert_worlds_equal(v, rv, "velocities")
    _assert_worlds_equal(gp, rtp, "tracer positions")
    _assert_worlds_equal(gv, rtv, "tracer velocities")
    assert not np.array_equal(gp[0], tp[0])
    if (n, m) == (65, 600):  # and a World of each world alone, with its tracers
        for k in range(3):
            world = nb.World(pos[k], vel[k], w[k], method="direct", arith="exact", tracers=(tp[k], tv[k]))
            try:
                world.update(DT, None, n_steps=3)
                wp, wv = world.tracers()
                bp, bv = world.particles()[:2]
            finally:
                world.close()
            assert _same_bits(gp[k], wp) and _same_bits(gv[k], wv), k
            assert _same_bits(p[k], bp) and _same_bits(v[k], bv), k


# ------------------------------------------------------------------ 2. tile edges
@pytest.mark.parametrize("m", [1, 255, 256, 257, 511, 513, 1023, 1025, 2049])
def test_tile_edges(nb, orc, m):
    """Every m around a multiple of the block, for any number of tracers per lane up to 8: EXACT against the oracle, and FAST
    against itself with m halved (the first half of the tracers alone: other tiles, other lanes, the same bits)."""
    n = 7
    pos, vel, w = _worlds(nb, n, 2, seed=1200, awkward_at=-1)
    tp, tv = _tracers_for(pos, m, 2100 + m)
    p, v, gp, gv = _run(nb, pos, vel, w, (tp, tv), "exact", calls=(1,))
    rp, rv, rtp, rtv = _exact_steps(orc, pos, vel, w, tp, tv, 1)
    _assert_worlds_equal(p, rp, "positions")
    _assert_worlds_equal(gp, rtp, "tracer positions")
    _assert_worlds_equal(gv, rtv, "tracer velocities")
    h = max(1, m // 2)
    with nb.RestrictedEnsemble(pos, vel, w, (tp, tv), arith="fast") as r:
        full = r.tracers_accel()
        r.set_tracers((tp[:, :h], tv[:, :h]))
        half = r.tracers_accel()
    assert full.shape == (2, m, 2) and half.shape == (2, h, 2)
    assert _same_bits(full[:, :h], half)
    inside = ~np.stack([_outside_fast(tp[k]) for k in range(2)])
    assert np.all(np.isfinite(full[inside])) and np.any(full[inside] != 0)


# ------------------------------------------------------------------ 3. the bodies never notice
@pytest.mark.parametrize("arith", ["exact", "fast", "auto"])
def test_bodies_are_the_ensembles_with_and_without_tracers(nb, arith):
    n = 300
    pos, vel, w = _worlds(nb, n, 3, seed=1300, awkward_at=1)
    tp, tv = _tracers_for(pos, 600, 2200)
    with nb.Ensemble(pos, vel, w, arith=arith) as ens:
        ens.update(DT, None, n_steps=3)
        ep, ev, _ = ens.particles()
        ea = ens.accel()
    for tracers in (None, (tp, tv)):
        with nb.RestrictedEnsemble(pos, vel, w, tracers, arith=arith) as r:
            assert r.shape == (3, n, 0 if tracers is None else 600)
            r.update(DT, None, n_steps=3)
            p, v, _ = r.particles()
            a = r.accel()
        _assert_worlds_equal(p, ep, f"positions, tracers {tracers is not None}")
        _assert_worlds_equal(v, ev, f"velocities, tracers {tracers is not None}")
        _assert_worlds_equal(a, ea, f"accelerations, tracers {tracers is not None}")


# ------------------------------------------------------------------ 4. FAST within the frozen tolerance
@pytest.fixture(scope="module")
def galaxy(nb):
    return nb.scenes.galaxy()


@pytest.mark.parametrize("n", [2, 64, 1000, 4096])
def test_fast_tracers_within_the_frozen_tolerance(nb, orc, galaxy, n):
    pos, vel, w = _fast_worlds(nb, galaxy, n)
    tp, tv = _tracers_for(pos, 600, 2300 + n, with_skip=False)  # all finite: on, near and away from bodies
    assert np.all(np.isfinite(tp))
    with nb.RestrictedEnsemble(pos, vel, w, (tp, tv), arith="fast") as r:
        acc = r.tracers_accel()
    ran_fast = False
    for k in range(3):
        ref64, norm = orc.direct_accel(pos[k], w[k], target_pos=tp[k], accum="f64", nthreads=NTH)
        cpu32, _ = orc.direct_accel(pos[k], w[k], target_pos=tp[k], accum="native", nthreads=NTH)
        check_fast(acc[k], ref64, norm, cpu32, label=f" n={n} world {k}")
        ran_fast |= not np.array_equal(acc[k], cpu32.astype(F32))
    assert ran_fast


# ------------------------------------------------------------------ 5. a tracer on a body sees what the body sees
@pytest.mark.parametrize("n", [129, 300, 4096])
def test_fast_a_tracer_on_a_body_gets_the_bodys_bits(nb, n):
    pos, vel, w = _worlds(nb, n, 3, seed=1500 + n, awkward_at=-1)
    assert np.all(np.isfinite(pos))
    with nb.Ensemble(pos, vel, w, arith="fast") as ens:
        body = ens.accel()
    with nb.RestrictedEnsemble(pos, vel, w, (pos.copy(), vel.copy()), arith="fast") as r:
        tracer = r.tracers_accel()
    assert body.shape == tracer.shape == (3, n, 2)
    for k in range(3):
        assert body[k].tobytes() == tracer[k].tobytes(), k
    assert np.any(body != 0)


# ------------------------------------------------------------------ 6. independence
@pytest.mark.parametrize("arith", ["exact", "fast", "auto"])
def test_a_tracer_depends_on_its_own_state_and_its_worlds_bodies_alone(nb, arith):
    n, b, m = 300, 5, 600
    pos, vel, w = _worlds(nb, n, b, seed=1600, awkward_at=3)  # (under AUTO world 3 routes to EXACT, its neighbours do not)
    tp, tv = _tracers_for(pos, m, 2400)                       # (the skip cases at the end: AUTO's per-tracer exception)
    ref = _run(nb, pos, vel, w, (tp, tv), arith)
    assert not np.array_equal(ref[2], tp)
    # in another slot: the tracers of every world reversed
    got = _run(nb, pos, vel, w, (tp[:, ::-1], tv[:, ::-1]), arith)
    assert _same_bits(got[2][:, ::-1], ref[2]) and _same_bits(got[3][:, ::-1], ref[3])
    # at another world index, with other contents in the worlds around it
    got = _run(nb, pos[::-1], vel[::-1], w[::-1], (tp[::-1], tv[::-1]), arith)
    for x, y in zip(got, ref):
        assert _same_bits(x[::-1], y)
    # 3 steps as one call against 1 + 2
    got = _run(nb, pos, vel, w, (tp, tv), arith, calls=(1, 2))
    for x, y in zip(got, ref):
        assert _same_bits(x, y)
    # B = 1 against 5, and m = 1 against 600: one tracer of one world, alone
    for k, i in ((0, 0), (3, 17), (4, m - 1), (2, 256), (3, m - 8)):
        got = _run(nb, pos[k:k + 1], vel[k:k + 1], w[k:k + 1], (tp[k:k + 1, i:i + 1], tv[k:k + 1, i:i + 1]), arith)
        assert _same_bits(got[2][0, 0], ref[2][k, i]) and _same_bits(got[3][0, 0], ref[3][k, i]), (k, i)
        assert _same_bits(got[0][0], ref[0][k]) and _same_bits(got[1][0], ref[1][k]), k


# ------------------------------------------------------------------ 7. AUTO
def test_auto_a_nan_body_makes_its_world_exact_and_no_other(nb, orc):
    n, m = 200, 600
    pos, vel, w = _worlds(nb, n, 3, seed=1700, awkward_at=-1)
    pos[1, 7] = (np.nan, 3.0)
    tp, tv = _tracers_for(pos, m, 2500, with_skip=False)
    p, v, gp, gv = _run(nb, pos, vel, w, (tp, tv), "auto", calls=(2,))
    rp, rv, rtp, rtv = _exact_steps(orc, pos, vel, w, tp, tv, 2)
    assert _same_bits(p[1], rp[1]) and _same_bits(v[1], rv[1])
    assert _same_bits(gp[1], rtp[1]) and _same_bits(gv[1], rtv[1])
    fast = _run(nb, pos, vel, w, (tp, tv), "fast", calls=(2,))
    for k in (0, 2):
        for x, y in zip((p, v, gp, gv), fast):
            assert x[k].tobytes() == y[k].tobytes(), k
    # the routes themselves, in the accelerations at the initial state: world 1 EXACT, its neighbours not
    with nb.RestrictedEnsemble(pos, vel, w, (tp, tv), arith="auto") as r:
        acc = r.tracers_accel()
    ex = _exact_accel(orc, pos, w, tp)
    for k in range(3):
        assert _same_bits(acc[k], ex[k]) == (k == 1), k


def test_auto_a_tracer_outside_the_domain_takes_its_exact_value(nb, orc):
    n, m = 200, 700
    pos, vel, w = _worlds(nb, n, 2, seed=1710, awkward_at=-1)
    tp, tv = _tracers_for(pos, m, 2510, with_skip=False)
    tp[0, 300] = (2.0 ** 61, 3.0)
    tp[1, 511] = (50000.0, 1e-8)
    odd = np.zeros((2, m), bool)
    odd[0, 300] = odd[1, 511] = True
    with nb.RestrictedEnsemble(pos, vel, w, (tp, tv), arith="auto") as r:
        auto = r.tracers_accel()
    with nb.RestrictedEnsemble(pos, vel, w, (tp, tv), arith="fast") as r:
        fast = r.tracers_accel()
    ex = _exact_accel(orc, pos, w, tp)
    assert _same_bits(auto[odd], ex[odd])
    assert auto[~odd].tobytes() == fast[~odd].tobytes()
    assert not _same_bits(auto[0, :300], ex[0, :300]) and not _same_bits(auto[1, :511], ex[1, :511])  # the others ran FAST
    # a clamp below FAST's floor: everything EXACT
    p, v, gp, gv = _run(nb, pos, vel, w, (tp, tv), "auto", calls=(2,), clamp=1e-7)
    rp, rv, rtp, rtv = _exact_steps(orc, pos, vel, w, tp, tv, 2, clamp=1e-7)
    for x, y, what in ((p, rp, "positions"), (v, rv, "velocities"), (gp, rtp, "tracer positions"), (gv, rtv, "tracer velocities")):
        _assert_worlds_equal(x, y, "clamp 1e-7 " + what)


def test_auto_a_tracer_that_crosses_the_domain_boundary_is_routed_once_per_step(nb, orc):
    """The route of a tracer in a step is decided from its pre-step position.  Reference, step by step: FAST's bits (the handle
    under FAST by name) where the pre-step position is inside the domain, the oracle's sum where it is outside, then Euler."""
    n = 200
    pos, vel, w = _worlds(nb, n, 2, seed=1720, awkward_at=-1)
    fp, fv = _tracers_for(pos, 500, 2520, with_skip=False)
    xp, xv = _crossing_tracers(F32)
    tp = np.concatenate([fp[:, :250], np.stack([xp, xp]), fp[:, 250:]], axis=1)
    tv = np.concatenate([fv[:, :250], np.stack([xv, xv]), fv[:, 250:]], axis=1)
    steps = 3
    p, v, gp, gv = _run(nb, pos, vel, w, (tp, tv), "auto", calls=(steps,))
    rtp, rtv = tp, tv
    went_out = came_in = 0
    with nb.Ensemble(pos, vel, w, arith="auto") as bodies:
        for _ in range(steps):
            bp, bv, _ = bodies.particles()
            with nb.RestrictedEnsemble(bp, bv, w, (rtp, rtv), arith="fast") as r:
                a = r.tracers_accel()
            out = np.stack([_outside_fast(rtp[k]) for k in range(2)])
            a[out] = _exact_accel(orc, bp, w, rtp)[out]
            rtp, rtv = _euler(rtp, rtv, a, DT)
            after = np.stack([_outside_fast(rtp[k]) for k in range(2)])
            went_out += int(np.sum(~out & after))
            came_in += int(np.sum(out & ~after))
            bodies.update(DT, None, n_steps=1)
        bp, bv, _ = bodies.particles()
    assert went_out >= 4 and came_in >= 4, (went_out, came_in)  # two of each per world: the cases this test is about did occur
    assert _same_bits(gp, rtp) and _same_bits(gv, rtv)
    assert p.tobytes() == bp.tobytes() and v.tobytes() == bv.tobytes()


# ------------------------------------------------------------------ 8. lifetime and errors
def test_lifetime_download_order_and_errors(nb, orc):
    C = nb._capi
    n, m = 65, 300
    pos, vel, w = _worlds(nb, n, 3, seed=1800, awkward_at=-1)
    tp, tv = _tracers_for(pos, m, 2600, with_skip=False)
    with nb.RestrictedEnsemble(pos, vel, w, (tp, tv), arith="exact") as r:
        gp, gv = r.tracers()                                    # download keeps upload order
        assert gp.tobytes() == tp.tobytes() and gv.tobytes() == tv.tobytes()
        a = r.accel()                                           # accel() and tracers_accel() leave the state's bits alone
        ta = r.tracers_accel()
        assert _same_bits(ta, _exact_accel(orc, pos, w, tp)) and a.shape == (3, n, 2)
        p, v, _ = r.particles()
        gp, gv = r.tracers()
        assert p.tobytes() == pos.tobytes() and v.tobytes() == vel.tobytes()
        assert gp.tobytes() == tp.tobytes() and gv.tobytes() == tv.tobytes()
        # set_tracers replaces (another m), and m = 0 removes
        r.set_tracers((tp[:, :7], tv[:, :7]))
        assert r.shape == (3, n, 7)
        r.update(DT, None, n_steps=2)
        gp, gv = r.tracers()
        rp, rv, rtp, rtv = _exact_steps(orc, pos, vel, w, tp[:, :7], tv[:, :7], 2)
        _assert_worlds_equal(gp, rtp, "replaced tracers")
        _assert_worlds_equal(r.particles()[0], rp, "bodies")
        r.set_tracers((tp[:, :0], tv[:, :0]))
        assert r.shape == (3, n, 0) and r.tracers()[0].shape == (3, 0, 2) and r.tracers_accel().shape == (3, 0, 2)
        r.update(DT, None, n_steps=1)
        _assert_worlds_equal(r.particles()[0], _oracle_steps(orc, rp, rv, w, 1)[0], "bodies without tracers")
        r.set_tracers((tp, tv))
        assert r.shape == (3, n, m)
        r.set_tracers(None)
        assert r.shape == (3, n, 0)
        # a body upload removes the tracers
        r.set_tracers((tp, tv))
        r.upload(pos[:2], vel[:2], w[:2])
        assert r.shape == (2, n, 0)
        # the C level: a tracer B mismatch, a NULL array with m > 0
        for call in (lambda: r.h.upload_tracers(3, m, tp, tv), lambda: r.h.upload_tracers(2, m, None, tv[:2]),
                     lambda: r.h.upload_tracers(2, m, tp[:2], None), lambda: r.h.upload_tracers(2, -1, tp[:2], tv[:2]),
                     lambda: r.h.upload_tracers(2, (1 << 25) + 1, tp[:2], tv[:2])):
            with pytest.raises(C.NBodyError) as e:
                call()
            assert e.value.code == C.ERR_INVALID and "restricted" in str(e.value)
        assert r.shape == (2, n, 0)
        r.h.upload_tracers(2, 0, None, None)                    # m = 0 needs no arrays
    h = C.RestrictedHandle(0)
    try:
        assert h.shape == (0, 0) and h.n_tracers == 0
        for call in (lambda: h.update(DT, 1), h.accel, h.download, h.tracers_accel, h.download_tracers,
                     lambda: h.upload_tracers(1, 4, tp[0, :4], tv[0, :4]),
                     lambda: h.upload(1, 4097, np.zeros((4097, 2), F32), np.zeros((4097, 2), F32), None)):
            with pytest.raises(C.NBodyError) as e:
                call()
            assert e.value.code == C.ERR_INVALID and "restricted" in str(e.value)
        assert h.shape == (0, 0)
    finally:
        h.close()
    cnt = nb.Counting()
    with nb.RestrictedEnsemble(pos, vel, w, (tp, tv)) as r:    # booking: the whole call under sum_gravity
        r.update(DT, cnt, n_steps=0)
        assert cnt.sum_gravity == 0.0
        r.update(DT, cnt, n_steps=2)
        assert cnt.sum_gravity > 0.0 and cnt.build_bvh == 0.0 and cnt.post_calculations == 0.0


def test_a_refused_upload_leaves_bodies_and_tracers_as_they_were(nb, orc):
    """An upload refused for its arguments changes nothing.  The C call on the handle itself: the Python class would refuse first."""
    C = nb._capi
    n, m = 3, 5
    pos, vel, w = _worlds(nb, n, 2, seed=1900, awkward_at=-1)
    tp, tv = _tracers_for(pos, m, 2700, with_skip=False)
    big = np.zeros((2, 4097, 2), F32)
    with nb.RestrictedEnsemble(pos, vel, w, (tp, tv), arith="exact") as r:
        r.update(DT, None, n_steps=1)
        before = (*r.h.download(), *r.h.download_tracers())
        assert not np.array_equal(before[0], pos) and not np.array_equal(before[2], tp)
        for call in (lambda: r.h.upload(2, 4097, big, big, None), lambda: r.h.upload(2, n, None, vel, w)):
            with pytest.raises(C.NBodyError) as e:
                call()
            assert e.value.code == C.ERR_INVALID
            assert r.h._call("_last_error").decode().startswith("restricted upload:")
            assert r.h.shape == (2, n) and r.h.n_tracers == m
        after = (*r.h.download(), *r.h.download_tracers())
        for x, y in zip(after, before):
            assert x.shape == y.shape and x.tobytes() == y.tobytes()
        r.update(DT, None, n_steps=1)
        p, v, _ = r.particles()
        gp, gv = r.tracers()
    rp, rv, rtp, rtv = _exact_steps(orc, pos, vel, w, tp, tv, 2)
    for x, y, what in ((p, rp, "positions"), (v, rv, "velocities"), (gp, rtp, "tracer positions"), (gv, rtv, "tracer velocities")):
        _assert_worlds_equal(x, y, what)
