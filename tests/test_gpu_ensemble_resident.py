"""Resident runs on the device (run() of Ensemble, Ensemble64, RaggedEnsemble, RaggedEnsemble64 over nbody_resident_*): a sweep
whose worlds stay in LDS for up to 1024 steps of a launch.  Every comparison is bitwise, in words of uint32 or uint64: against
sweep() on a twin handle, against update(), against the same class holding a world alone, and under EXACT against the oracle's
update_direct of every world under its own delta, clamp and nsteps.  The scenes are tests/_resident_scene.py's.  Needs an MI355X."""
import functools

import numpy as np
import pytest

from _resident_scene import (B, CLAMP, DELTA, FLOOR, NTH, STEPS, STILL, assert_same, cls_of, outside_fast, same, scene, specials,
                             world)

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 255, 256]     # every edge of the lane split, and the full tile
ARITHS = [("float32", "exact"), ("float32", "fast"), ("float32", "auto"), ("float64", "exact"), ("float64", "fast")]


def _rows(e):
    p, v, _ = e.particles()
    return p, v


def _assert_rows(got, want, what):
    for name, g, w in zip(("positions", "velocities"), got, want):
        if isinstance(g, list):
            assert len(g) == len(w), what
            for k, (gk, wk) in enumerate(zip(g, w)):
                assert_same(gk, wk, f"{what}: {name} of world {k}")
        else:
            assert_same(g, w, f"{what}: {name}")


@functools.lru_cache(maxsize=None)
def _oracle_worlds(n, dtype_name):
    """The oracle's result of every world of scene(n) under its own delta, clamp and nsteps: computed once, shared."""
    from oracle import oracle as orc
    pos, vel, w = scene(n, dtype_name)
    out = [orc.update_direct(pos[k], vel[k], w[k], delta=DELTA[k], clamp=CLAMP[k], nsteps=int(STEPS[k]), nthreads=NTH)[:2] for k in range(B)]
    rp, rv = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    rp.setflags(write=False), rv.setflags(write=False)
    return rp, rv


# ------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("dtype,arith", ARITHS)
@pytest.mark.parametrize("n", SIZES)
def test_run_is_the_sweep_at_every_size_and_exact_is_the_oracle(nb, orc, n, dtype, arith):
    pos, vel, w = scene(n, dtype)
    assert CLAMP[2] < FLOOR <= CLAMP[1] and CLAMP[1] != CLAMP[2]          # neighbours, one of them below the floor of f32 FAST
    cls = cls_of(nb, dtype)
    with cls(pos, vel, w, arith=arith, clamp=0.5) as e, cls(pos, vel, w, arith=arith, clamp=0.5) as twin:   # (the handle's clamp is no world's)
        e.run(DELTA, clamp=CLAMP, steps=STEPS, n_steps=4)
        twin.sweep(DELTA, CLAMP, STEPS, n_steps=4)
        got, want = _rows(e), _rows(twin)
    _assert_rows(got, want, f"{arith} n {n}")
    # the world of 0 steps keeps -0.0, the NaN's payload and the infinity
    assert_same(got[0][STILL], pos[STILL], "positions of the world of 0 steps")
    assert_same(got[1][STILL], vel[STILL], "velocities of the world of 0 steps")
    sp = specials(dtype)[:2 * n]
    assert_same(got[1][STILL].reshape(-1)[:len(sp)], sp, "the special values")
    assert not same(got[0][0], pos[0])
    if arith == "exact":
        rp, rv = _oracle_worlds(n, dtype)
        for k in range(B):
            assert_same(got[0][k], rp[k], f"n {n}: positions of world {k} against the oracle")
            assert_same(got[1][k], rv[k], f"n {n}: velocities of world {k} against the oracle")


# ------------------------------------------------------------------ 2. the route changes inside a call, both ways
ROUTE_STEPS = 6


def _route_scene(n, dtype):
    """Three worlds of n bodies under delta = 1.  World 0: body n - 1 has velocity 2^58 (f64: 2^98), so it is at 4 * 2^58 = 2^60 (2^100),
    the first coordinate outside FAST's domain, after 4 steps.  World 1: body n - 1 starts at 2^61 (2^101), outside, with velocity
    -2^59 (-2^99): 3 * 2^59, 2^60, then 2^59, inside after 3 steps.  World 2 stays inside."""
    t = np.dtype(dtype).type
    e = 58 if t is np.float32 else 98
    pos, vel, w = (a.copy() for a in scene(n, dtype, 3, False))
    vel[0, n - 1] = [t(2.0 ** e), 0]
    pos[1, n - 1] = [t(2.0 ** (e + 3)), 2.0]
    vel[1, n - 1] = [-t(2.0 ** (e + 1)), 0]
    return pos, vel, w


@pytest.mark.parametrize("dtype,arith", [("float32", "auto"), ("float64", "fast")])
@pytest.mark.parametrize("n", [3, 64, 128, 129])
def test_a_world_leaves_and_a_world_enters_fasts_domain_inside_a_call(nb, orc, n, dtype, arith):
    pos, vel, w = _route_scene(n, dtype)
    # before anything runs on the GPU: over the oracle's trajectory, world 0 is inside the domain at step 0 and outside at the
    # start of the last step, world 1 the reverse, and each changes once (if not, the scene is at fault, not the kernel)
    out = np.zeros((3, ROUTE_STEPS), bool)
    for k in range(3):
        p, v = pos[k], vel[k]
        for s in range(ROUTE_STEPS):
            out[k, s] = outside_fast(p).any()
            p, v, _ = orc.update_direct(p, v, w[k], delta=1.0, clamp=1e-3, nsteps=1, nthreads=NTH)
    assert not out[0, 0] and out[0, -1] and list(out[0]) == sorted(out[0]), out[0]
    assert out[1, 0] and not out[1, -1] and list(out[1]) == sorted(out[1], reverse=True), out[1]
    assert 0 < out[0].sum() < ROUTE_STEPS and 0 < out[1].sum() < ROUTE_STEPS and not out[2].any()
    cls = cls_of(nb, dtype)
    with cls(pos, vel, w, arith=arith) as e, cls(pos, vel, w, arith=arith) as twin, cls(pos, vel, w, arith="exact") as exact:
        e.run(1.0, n_steps=ROUTE_STEPS)
        twin.update(1.0, None, n_steps=ROUTE_STEPS)
        exact.update(1.0, None, n_steps=ROUTE_STEPS)
        got, want, other = _rows(e), _rows(twin), _rows(exact)
    _assert_rows(got, want, f"{arith} n {n}")
    # FAST steps were taken: world 0, whose first four steps are FAST while its bodies are still close, does not carry the bits of
    # EXACT throughout.  (World 1 may: by the time it turns FAST its bodies have scattered, and a FAST acceleration that differs
    # in its last bits from the EXACT one adds to a velocity 10^7 times its size.)
    if n >= 64:
        assert not same(got[1][0], other[1][0])


# ------------------------------------------------------------------ 3. the launch boundary
LONG = 1025
LONG_STEPS = np.array([0, 1, 1023, 1024, 1025, 1025], np.int32)
LONG_DELTA = DELTA * 0.01


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("arith", ["exact", "fast"])
@pytest.mark.parametrize("n", [3, 129])
def test_the_cut_into_launches_is_invisible(nb, n, arith, dtype):
    pos, vel, w = scene(n, dtype, B, False)
    plan = nb.resident_plan([n] * B, LONG_STEPS, LONG, dtype)
    assert plan["n_launches"] == 2
    cls = cls_of(nb, dtype)
    with cls(pos, vel, w, arith=arith) as e, cls(pos, vel, w, arith=arith) as twin, cls(pos, vel, w, arith=arith) as split:
        e.run(LONG_DELTA, clamp=CLAMP, steps=LONG_STEPS, n_steps=LONG)
        twin.sweep(LONG_DELTA, CLAMP, LONG_STEPS, n_steps=LONG)
        first = np.minimum(LONG_STEPS, 1024).astype(np.int32)
        split.run(LONG_DELTA, clamp=CLAMP, steps=first, n_steps=1024)
        split.run(LONG_DELTA, clamp=CLAMP, steps=LONG_STEPS - first, n_steps=1)
        got, want, cut = _rows(e), _rows(twin), _rows(split)
        streams, step = e.deltas()
    _assert_rows(got, want, f"{arith} n {n}: run against sweep")
    _assert_rows(cut, got, f"{arith} n {n}: run(1024) then run(1) against run(1025)")
    assert step == LONG
    assert_same(got[0][0], pos[0], "the world of 0 steps")


# ------------------------------------------------------------------ 4. independence
@pytest.mark.parametrize("dtype,arith", [("float32", "auto"), ("float32", "exact"), ("float64", "fast")])
@pytest.mark.parametrize("n", [3, 64, 129])
def test_a_world_does_not_depend_on_its_index_or_its_neighbours(nb, n, dtype, arith):
    pos, vel, w = scene(n, dtype)
    cls = cls_of(nb, dtype)
    with cls(pos, vel, w, arith=arith, clamp=0.5) as e:
        e.run(DELTA, clamp=CLAMP, steps=STEPS, n_steps=4)
        got = _rows(e)
    op, ov, ow = world(n, 31337 + n, dtype)             # a world that is none of the six
    with cls(pos[:2], vel[:2], w[:2], arith=arith, clamp=0.5) as pair, cls(pos[:1], vel[:1], w[:1], arith=arith, clamp=0.5) as alone:
        for k in range(B):
            alone.upload(pos[k:k + 1], vel[k:k + 1], w[k:k + 1])      # a handle holding world k alone
            alone.run([DELTA[k]], clamp=[CLAMP[k]], steps=[STEPS[k]], n_steps=4)
            p, v = _rows(alone)
            assert_same(p[0], got[0][k], f"{arith} n {n}: positions of world {k} alone")
            assert_same(v[0], got[1][k], f"{arith} n {n}: velocities of world {k} alone")
            pair.upload(np.stack([op, pos[k]]), np.stack([ov, vel[k]]), np.stack([ow, w[k]]))
            pair.run([0.3, DELTA[k]], clamp=[3e-3, CLAMP[k]], steps=[4, STEPS[k]], n_steps=4)
            p, v = _rows(pair)
            assert_same(p[1], got[0][k], f"{arith} n {n}: positions of world {k} at index 1 beside another world")
            assert_same(v[1], got[1][k], f"{arith} n {n}: velocities of world {k} at index 1 beside another world")


@pytest.mark.parametrize("dtype,arith", [("float32", "auto"), ("float64", "fast"), ("float64", "exact")])
@pytest.mark.parametrize("n", [5, 129])
def test_run_update_run_is_one_update(nb, n, dtype, arith):
    pos, vel, w = scene(n, dtype, B, False)
    cls = cls_of(nb, dtype)
    with cls(pos, vel, w, arith=arith) as e, cls(pos, vel, w, arith=arith) as whole:
        e.run(0.1, n_steps=3)
        e.update(0.1, None, n_steps=2)
        e.run(0.1, n_steps=4)
        whole.update(0.1, None, n_steps=9)
        got, want = _rows(e), _rows(whole)
        assert e.deltas()[1] == whole.deltas()[1] == 9
    _assert_rows(got, want, f"{arith} n {n}")
    assert not same(got[0], pos)


# ------------------------------------------------------------------ 5. ragged
RSIZES = [1, 3, 64, 65, 128, 129, 256]
RDELTA = np.array([0.13, 0.4, 0.1, 0.2, 0.05, 0.07, 0.11])
RCLAMP = np.array([1e-3, 1e-2, 1e-6, 1e-3, 1e-2, 2.5e-4, 1e-3], np.float32)
RSTEPS = np.array([3, 1, 4, 2, 0, 4, 3], np.int32)


@pytest.mark.parametrize("arith", ["exact", "fast", "auto"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_ragged_worlds_are_the_sweep_and_the_worlds_alone(nb, dtype, arith):
    worlds = [world(n, 9500 + k, dtype) for k, n in enumerate(RSIZES)]
    ps, vs, ws = ([x[i] for x in worlds] for i in range(3))
    cls, one = cls_of(nb, dtype, "RaggedEnsemble"), cls_of(nb, dtype)
    plan = nb.resident_plan(RSIZES, RSTEPS, 4, dtype)
    assert plan == dict(n_launches=1, lds_bytes=128 * 24 + 256 * 8 if dtype == "float32" else 256 * 20 + 256 * 16)
    with cls(ps, vs, ws, arith=arith, clamp=0.5) as e, cls(ps, vs, ws, arith=arith, clamp=0.5) as twin:
        e.run(RDELTA, clamp=RCLAMP, steps=RSTEPS, n_steps=4)
        twin.sweep(RDELTA, RCLAMP, RSTEPS, n_steps=4)
        got, want = _rows(e), _rows(twin)
    _assert_rows(got, want, f"{arith}: run against sweep")
    for k in range(len(RSIZES)):
        with one(ps[k], vs[k], ws[k], arith=arith, clamp=float(RCLAMP[k])) as single:
            single.run(float(RDELTA[k]), n_steps=int(RSTEPS[k]))
            p, v = _rows(single)
        assert_same(got[0][k], p[0], f"{arith}: positions of world {k} against the world alone")
        assert_same(got[1][k], v[0], f"{arith}: velocities of world {k} against the world alone")
    assert_same(got[0][4], ps[4], "the world of 0 steps")
    assert not same(got[0][6], ps[6])


# ------------------------------------------------------------------ 6. what the handle remembers
@pytest.mark.parametrize("kind", ["Ensemble", "Ensemble64", "RaggedEnsemble", "RaggedEnsemble64"])
def test_delta_streams_summaries_and_encounters_after_a_run_are_the_sweeps(nb, kind):
    dtype = "float64" if kind.endswith("64") else "float32"
    if kind.startswith("Ragged"):
        worlds = [world(n, 9700 + k, dtype) for k, n in enumerate([5, 65, 3, 129, 17, 256])]
        args = tuple([x[i] for x in worlds] for i in range(3))
    else:
        args = scene(65, dtype)
    cls = getattr(nb, kind)
    with cls(*args, arith="auto") as e, cls(*args, arith="auto") as twin:
        for h in (e, twin):
            h.deltas()                                           # key frames: the sequence begins
            h.update(0.1, None, n_steps=2)
            h.deltas()
        e.run(DELTA, clamp=CLAMP, steps=STEPS, n_steps=4)
        twin.sweep(DELTA, CLAMP, STEPS, n_steps=4)
        (gs, gstep), (ws, wstep) = e.deltas(), twin.deltas()
        assert gstep == wstep == 6
        assert gs == ws                                          # byte for byte, the step number in the headers included
        for k, s in enumerate(gs):
            assert int.from_bytes(s[16:24], "little") == 6, k
        assert e.summary(height=8).tobytes() == twin.summary(height=8).tobytes()
        ge, we = e.encounters(), twin.encounters()
        assert ge[0].tobytes() == we[0].tobytes()
        for g, w in zip(ge[1:], we[1:]):
            g, w = (np.concatenate(x) if isinstance(x, list) else x for x in (g, w))
            assert_same(g, w, "encounters' rows")
        e.update(0.1, None, n_steps=1)                            # and the next delta stream follows on both alike
        twin.update(0.1, None, n_steps=1)
        assert e.deltas() == twin.deltas()
        _assert_rows(_rows(e), _rows(twin), kind)


# ------------------------------------------------------------------ 7. refusals
def _refused(C, handle, call, word, what):
    """`call` is refused with NBODY_ERR_INVALID, and the library's own message on `handle` begins with the handle's word."""
    with pytest.raises(C.NBodyError) as err:
        call()
    assert err.value.code == C.ERR_INVALID
    msg = handle._call("_last_error").decode()
    assert msg.startswith(word + " resident") and what in msg and msg in str(err.value), msg


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_refusals_name_the_handle_and_resident_and_nothing_moves(nb, dtype):
    C = nb._capi
    delta = np.ascontiguousarray(DELTA, dtype=dtype)
    pos, vel, w = (np.stack([world(257, 8800 + k, dtype)[i] for k in range(B)]) for i in range(3))
    with cls_of(nb, dtype)(pos, vel, w, arith="auto") as e:
        _refused(C, e.h, lambda: e.run(DELTA, clamp=CLAMP, steps=STEPS), "ensemble", "257")
        _refused(C, e.h, lambda: e.run(0.1, n_steps=0), "ensemble", "257")              # (the checks come before the no-op)
        _assert_rows(_rows(e), (pos, vel), "a uniform handle of 257 bodies")
        assert e.deltas()[1] == 0
        fresh = type(e.h)(0)                                                        # a handle with nothing uploaded
        try:
            _refused(C, fresh, lambda: fresh.resident(delta, CLAMP, STEPS, 4), "ensemble", "nothing uploaded")
        finally:
            fresh.close()
    worlds = [world(n, 8900 + k, dtype) for k, n in enumerate([5, 256, 257, 3, 300, 64])]
    ps, vs, ws = ([x[i] for x in worlds] for i in range(3))
    with cls_of(nb, dtype, "RaggedEnsemble")(ps, vs, ws, arith="auto") as r:
        _refused(C, r.h, lambda: r.run(DELTA, clamp=CLAMP, steps=STEPS), "ragged", "world 2")
        _assert_rows(_rows(r), (ps, vs), "a ragged handle whose world 2 has 257 bodies")
        fresh = type(r.h)(0)
        try:
            _refused(C, fresh, lambda: fresh.resident(delta, CLAMP, STEPS, 4), "ragged", "nothing uploaded")
        finally:
            fresh.close()
        # the sweep's refusals, under the run's name; and the handle still works
        r.upload(ps[:2], vs[:2], ws[:2])
        _refused(C, r.h, lambda: r.h.resident(None, None, None, 1), "ragged", "delta")
        _refused(C, r.h, lambda: r.h.resident(delta[:2], None, None, -1), "ragged", "n_steps")
        _refused(C, r.h, lambda: r.h.resident(delta[:2], None, np.array([1, 3], np.int32), 2), "ragged", "world 1")
        r.h.resident(delta[:2], None, np.zeros(2, np.int32), 0)                     # n_steps == 0 after the checks: a no-op
        _assert_rows(_rows(r), (ps[:2], vs[:2]), "n_steps == 0")
        r.run(0.1, n_steps=2)
        assert not same(_rows(r)[0][1], ps[1]) and r.deltas()[1] == 2
