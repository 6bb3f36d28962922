"""Sweeps on the device (sweep() of the eight ensemble classes over nbody_sweep_*): a time step, a clamp and a number of steps per
world.  Every comparison is bitwise.  EXACT worlds are compared with the oracle's update_direct of that world under its own
delta, clamp and nsteps (tracers: direct_accel at them + Euler); FAST and AUTO worlds with a handle of the same class holding
that world alone, set to the world's clamp and stepped by update(delta[k], n_steps=steps[k]).  Needs an MI355X.

Scenes.  Bodies in the box [1, 5)^2 (inside FAST's domain in both precisions), integer masses 1 .. 11, and in every world of two
or more bodies a planted pair 2^-10 apart: d^2 = 9.5e-7 is below every clamp used here (1e-2, 1e-3, 2.5e-4, 4e-6), so the pair's
term is another number under each of them.  Before anything runs on the GPU `_scene_is_telling` checks on the CPU, with the
oracle, that every world has such a pair and that one oracle step of world k under its neighbour's delta, and under its
neighbour's clamp, differs from the step under its own: a kernel that applies another world's parameters, or the handle's,
cannot pass.  (A world of one body has no pair and feels no clamp: for n = 1 only the delta is required to tell.)

Parameters.  Six worlds, pairwise distinct deltas, neighbouring worlds with different clamps, step counts from 0 to n_steps."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
NTH = 16
B = 6
DELTA = np.array([0.13, 0.4, 0.1, 0.2, 0.05, 0.07])
CLAMP = np.array([1e-3, 1e-2, 4e-6, 1e-3, 1e-2, 2.5e-4], np.float32)
STEPS = np.array([3, 1, 4, 2, 0, 4], np.int32)          # of n_steps = 4
SIZES = [1, 2, 3, 4, 5, 8, 9, 64, 65, 128, 129, 256, 257, 4096]   # the edges of every lane split and tile
FLOOR = np.float32(1.9073486328125e-06)                  # kFastClampFloor, 2^-19
PAIR = 2.0 ** -10


def _steps_for(n):
    """The step counts of a case: 0 .. 4 of n_steps = 4; the top size takes at most 2 (its oracle is 16.8 M pairs a step)."""
    steps = np.minimum(STEPS, 2) if n == 4096 else STEPS
    return steps.astype(np.int32), int(steps.max())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _assert_same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    word = np.uint32 if got.dtype == np.float32 else np.uint64
    diff = int((got.view(word) != want.view(word)).sum())
    assert diff == 0, f"{what}: {diff} of {got.size} words differ"


def _world(n, seed, dtype):
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 2)) * 4 + 1).astype(dtype)
    if n >= 2:
        pos[1] = pos[0] + np.array([PAIR, 0], dtype)
    vel = (rng.standard_normal((n, 2)) * 0.1).astype(dtype)
    w = ((np.arange(n) * (seed % 7 + 3)) % 11 + 1).astype(np.uint32)
    return pos, vel, w


@functools.lru_cache(maxsize=None)
def _scene(n, dtype_name, worlds=B):
    """`worlds` worlds of n bodies -> (pos[B, n, 2], vel[B, n, 2], w[B, n]), read-only and shared between the tests."""
    dtype = np.dtype(dtype_name).type
    parts = [_world(n, 7000 + 13 * n + k, dtype) for k in range(worlds)]
    out = tuple(np.stack([p[i] for p in parts]) for i in range(3))
    for a in out:
        a.setflags(write=False)
    return out


_TOLD = set()


def _scene_is_telling(orc, pos, vel, w, delta, clamp, key=None):
    """The CPU check of the module's docstring, once per scene and parameter set (`key`)."""
    if key is not None and key in _TOLD:
        return
    worlds = len(pos)
    for k in range(worlds):
        p, v, m = pos[k], vel[k], w[k]
        n = p.shape[0]
        if n >= 2:
            d = p[:, None, :].astype(np.float64) - p[None, :, :].astype(np.float64) if n <= 512 else (p[1] - p[0])[None, None, :].astype(np.float64)
            d2 = (d * d).sum(-1)
            close = d2[d2 > 0].min()
            assert close < float(min(clamp)), (k, close)                      # a pair closer than sqrt(clamp) of the smaller clamps
        nk = (k + 1) % worlds
        own = orc.update_direct(p, v, m, delta=delta[k], clamp=clamp[k], nsteps=1, nthreads=NTH)
        other_dt = orc.update_direct(p, v, m, delta=delta[nk], clamp=clamp[k], nsteps=1, nthreads=NTH)
        assert not _same(own[0], other_dt[0]) and delta[k] != delta[nk], k
        if n >= 2:
            other_clamp = orc.update_direct(p, v, m, delta=delta[k], clamp=clamp[nk], nsteps=1, nthreads=NTH)
            assert not _same(own[1], other_clamp[1]) and clamp[k] != clamp[nk], k
    if key is not None:
        _TOLD.add(key)


@functools.lru_cache(maxsize=None)
def _oracle_worlds(n, dtype_name):
    """The oracle's result of every world of _scene(n) under its own delta, clamp and nsteps: computed once, shared."""
    from oracle import oracle as orc
    pos, vel, w = _scene(n, dtype_name)
    steps, _ = _steps_for(n)
    out = [orc.update_direct(pos[k], vel[k], w[k], delta=DELTA[k], clamp=CLAMP[k], nsteps=int(steps[k]), nthreads=NTH)[:2] for k in range(B)]
    rp, rv = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    rp.setflags(write=False), rv.setflags(write=False)
    return rp, rv


def _cls(nb, dtype_name, kind="Ensemble"):
    return getattr(nb, kind + ("64" if dtype_name == "float64" else ""))


def _alone(single, k, pos, vel, w, delta, clamp, steps):
    """World k alone on the one-world handle `single` of the same class: set_params(clamp=clamp[k]), update(delta[k], steps[k])."""
    single.upload(pos[k:k + 1], vel[k:k + 1], w[k:k + 1])
    single.h.set_params(clamp=float(np.float32(clamp[k])))
    single.update(float(delta[k]), None, n_steps=int(steps[k]))
    p, v, _ = single.particles()
    return p[0], v[0]


# ------------------------------------------------------------------ 1. EXACT against the oracle, per world
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n", SIZES)
def test_exact_every_world_is_its_oracle_under_its_own_parameters(nb, orc, n, dtype):
    pos, vel, w = _scene(n, dtype)
    steps, n_steps = _steps_for(n)
    _scene_is_telling(orc, pos, vel, w, DELTA, CLAMP, key=(n, dtype))
    rp, rv = _oracle_worlds(n, dtype)
    with _cls(nb, dtype)(pos, vel, w, arith="exact", clamp=0.5) as e:     # (the handle's clamp is none of the worlds')
        e.sweep(DELTA, CLAMP, steps)
        p, v, _ = e.particles()
    assert p.dtype == np.dtype(dtype)
    for k in range(B):
        _assert_same(p[k], rp[k], f"n {n}: positions of world {k}")
        _assert_same(v[k], rv[k], f"n {n}: velocities of world {k}")
    _assert_same(p[4], pos[4], "the world of 0 steps")
    assert n_steps <= 4


# ------------------------------------------------------------------ 2. FAST and AUTO against the world alone
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("arith", ["fast", "auto"])
@pytest.mark.parametrize("n", SIZES)
def test_fast_and_auto_every_world_is_the_world_alone(nb, orc, n, arith, dtype):
    pos, vel, w = _scene(n, dtype)
    steps, _ = _steps_for(n)
    _scene_is_telling(orc, pos, vel, w, DELTA, CLAMP, key=(n, dtype))
    cls = _cls(nb, dtype)
    with cls(pos, vel, w, arith=arith, clamp=0.5) as e, cls(pos[:1], vel[:1], w[:1], arith=arith) as single:
        e.sweep(DELTA, CLAMP, steps)
        p, v, _ = e.particles()
        for k in range(B):
            ap, av = _alone(single, k, pos, vel, w, DELTA, CLAMP, steps)
            _assert_same(p[k], ap, f"{arith} n {n}: positions of world {k}")
            _assert_same(v[k], av, f"{arith} n {n}: velocities of world {k}")
    if arith == "fast" and n >= 64:      # FAST is another arithmetic than EXACT here: the comparison above is not vacuous
        _, rv = _oracle_worlds(n, dtype)
        assert not _same(v[0], rv[0])


# ------------------------------------------------------------------ 3. uniform arrays are the plain call
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("arith", ["exact", "fast", "auto"])
@pytest.mark.parametrize("n", [65, 257])
def test_uniform_arrays_are_the_plain_update(nb, n, arith, dtype):
    pos, vel, w = _scene(n, dtype)
    cls = _cls(nb, dtype)
    with cls(pos, vel, w, arith=arith) as a, cls(pos, vel, w, arith=arith) as b:
        a.update(0.1, None, n_steps=3)
        b.sweep(np.full(B, 0.1), clamp=None, steps=None, n_steps=3)
        (ap, av, _), (bp, bv, _) = a.particles(), b.particles()
    _assert_same(bp, ap, "positions")
    _assert_same(bv, av, "velocities")
    assert not _same(ap, pos)


# ------------------------------------------------------------------ 4. standing still
def _specials(dtype):
    """Rows whose bits no arithmetic hands back: -0.0, a NaN with a payload, +-inf, subnormals."""
    t = np.dtype(dtype).type
    if t is np.float32:
        nan, sub = np.array([0x7FC12345], np.uint32).view(np.float32)[0], np.float32(1e-41)
    else:
        nan, sub = np.array([0x7FF8000000012345], np.uint64).view(np.float64)[0], np.float64(1e-310)
    return np.array([[-0.0, 0.0], [nan, 2.0], [np.inf, -np.inf], [sub, -sub], [-0.0, nan]], dtype=t)


def _still_worlds(dtype, sizes):
    """Worlds of `sizes`; worlds 0 and 1 carry the special rows in positions and velocities."""
    t = np.dtype(dtype).type
    worlds = [list(_world(n, 8100 + k, t)) for k, n in enumerate(sizes)]
    sp = _specials(dtype)
    for k in (0, 1):
        worlds[k][0][7:7 + len(sp)] = sp
        worlds[k][1][40:40 + len(sp)] = sp
    return worlds


@pytest.mark.parametrize("n_steps", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["Ensemble", "Ensemble64", "RaggedEnsemble", "RaggedEnsemble64"])
def test_a_finished_world_stands_still_bit_for_bit(nb, kind, n_steps):
    """steps = 0, 1, 2, 3, n_steps, n_steps (capped at n_steps) under n_steps = 1 .. 4: a finished world is carried through
    one, two and three further launches, so through both parities of the position double buffer.  n = 257 is two tiles, the
    second nearly empty.  Under AUTO the worlds with non-finite rows take EXACT and the others FAST."""
    dtype = "float64" if kind.endswith("64") else "float32"
    ragged = kind.startswith("Ragged")
    sizes = [257, 129, 5, 600, 128, 64] if ragged else [257] * B
    worlds = _still_worlds(dtype, sizes)
    steps = np.minimum(np.array([0, 1, 2, 3, n_steps, n_steps]), n_steps).astype(np.int32)
    cls = getattr(nb, kind)
    ps, vs, ws = ([x[i] for x in worlds] for i in range(3))
    if ragged:
        with cls(ps, vs, ws, arith="auto") as e:
            e.sweep(DELTA, CLAMP, steps, n_steps=n_steps)
            p, v, _ = e.particles()
        single = cls(ps[:1], vs[:1], ws[:1], arith="auto")
    else:
        with cls(np.stack(ps), np.stack(vs), np.stack(ws), arith="auto") as e:
            e.sweep(DELTA, CLAMP, steps, n_steps=n_steps)
            p, v, _ = e.particles()
        single = cls(ps[0], vs[0], ws[0], arith="auto")
    with single:
        for k in range(B):
            if ragged:
                single.upload(ps[k:k + 1], vs[k:k + 1], ws[k:k + 1])
            else:
                single.upload(ps[k], vs[k], ws[k])
            single.h.set_params(clamp=float(CLAMP[k]))
            single.update(float(DELTA[k]), None, n_steps=int(steps[k]))
            ap, av, _ = single.particles()
            _assert_same(p[k], ap[0], f"positions of world {k} after its {steps[k]} of {n_steps} steps")
            _assert_same(v[k], av[0], f"velocities of world {k} after its {steps[k]} of {n_steps} steps")
    _assert_same(p[0], ps[0], "positions of the world of 0 steps: its upload")
    _assert_same(v[0], vs[0], "velocities of the world of 0 steps: its upload")
    assert not _same(p[5], ps[5])


# ------------------------------------------------------------------ 5. routing per world
def _pred(x):
    return np.nextafter(np.float32(x), np.float32(0))


@pytest.mark.parametrize("arith", ["fast", "auto"])
@pytest.mark.parametrize("n", [64, 129])
def test_f32_route_is_taken_per_world_from_its_clamp(nb, orc, n, arith):
    """Worlds 0 .. 2: a clamp one below kFastClampFloor, 0, NaN -> EXACT bits; worlds 3, 4: exactly the floor, 1e-3 -> FAST bits;
    world 5 (AUTO): a legal clamp and one position at 2^61, outside FAST's domain -> EXACT alone."""
    pos, vel, w = (a.copy() for a in _scene(n, "float32"))
    pos[5, 3] = [2.0 ** 61, 1.0]
    clamp = np.array([_pred(FLOOR), 0.0, np.nan, FLOOR, 1e-3, 1e-2], np.float32)
    steps = np.array([2, 2, 1, 2, 2, 2], np.int32)
    delta = DELTA
    E = nb.Ensemble
    with E(pos, vel, w, arith=arith) as e:
        e.sweep(delta, clamp, steps)
        p, v, _ = e.particles()
    with E(pos[:1], vel[:1], w[:1], arith="exact") as exact, E(pos[:1], vel[:1], w[:1], arith=arith) as same:
        for k in range(B):
            xp, xv = _alone(exact, k, pos, vel, w, delta, clamp, steps)
            # the route is visible: this world's FAST bits (under a clamp a FAST handle accepts) are not its EXACT bits
            legal = clamp.copy()
            legal[k] = clamp[k] if clamp[k] >= FLOOR else np.float32(1e-3)
            with E(pos[k:k + 1], vel[k:k + 1], w[k:k + 1], arith="fast", clamp=float(legal[k])) as fast:
                fast.update(float(delta[k]), None, n_steps=int(steps[k]))
                fp, fv, _ = fast.particles()
            xl = _alone(exact, k, pos, vel, w, delta, legal, steps)
            if k != 5:
                assert not _same(fv[0], xl[1]), f"world {k}: FAST and EXACT agree on this scene, the route would not show"
            if k in (0, 1, 2) or (k == 5 and arith == "auto"):
                _assert_same(p[k], xp, f"{arith}: world {k} (clamp {clamp[k]}) carries its EXACT positions")
                _assert_same(v[k], xv, f"{arith}: world {k} (clamp {clamp[k]}) carries its EXACT velocities")
            elif k in (3, 4):
                _assert_same(p[k], fp[0], f"{arith}: world {k} (clamp {clamp[k]}) carries its FAST positions")
                _assert_same(v[k], fv[0], f"{arith}: world {k} (clamp {clamp[k]}) carries its FAST velocities")
            sp, sv = _alone(same, k, pos, vel, w, delta, clamp, steps)
            _assert_same(p[k], sp, f"{arith}: world {k} is the world alone")
            _assert_same(v[k], sv, f"{arith}: world {k} is the world alone")
            if k in (0, 1):    # and the contract's yardstick, where the clamp is a number
                op, ov, _ = orc.update_direct(pos[k], vel[k], w[k], delta=delta[k], clamp=clamp[k], nsteps=int(steps[k]), nthreads=NTH)
                _assert_same(p[k], op, f"world {k} against the oracle")
                _assert_same(v[k], ov, f"world {k} against the oracle")


@pytest.mark.parametrize("n", [64, 129])
def test_f64_fast_is_taken_per_world_from_its_clamp(nb, orc, n):
    """Under FAST on Ensemble64: worlds with clamp 0, negative or NaN take EXACT, their neighbours (1e-3, 1e-2) FAST; world 5 has
    a legal clamp and a position at 2^101, outside the f64 FAST domain, and takes EXACT alone."""
    pos, vel, w = (a.copy() for a in _scene(n, "float64"))
    pos[5, 3] = [2.0 ** 101, 1.0]
    clamp = np.array([0.0, -1e-3, np.nan, 1e-3, 1e-2, 2.5e-4], np.float32)
    steps = np.array([2, 2, 1, 2, 2, 2], np.int32)
    E = nb.Ensemble64
    with E(pos, vel, w, arith="fast") as e:
        e.sweep(DELTA, clamp, steps)
        p, v, _ = e.particles()
    with E(pos[:1], vel[:1], w[:1], arith="exact") as exact, E(pos[:1], vel[:1], w[:1], arith="fast") as fast:
        for k in range(B):
            xp, xv = _alone(exact, k, pos, vel, w, DELTA, clamp, steps)
            legal = clamp.copy()
            legal[k] = clamp[k] if clamp[k] > 0 else np.float32(1e-3)
            fp, fv = _alone(fast, k, pos, vel, w, DELTA, legal, steps)
            xl = _alone(exact, k, pos, vel, w, DELTA, legal, steps)
            if k != 5:
                assert not _same(fv, xl[1]), f"world {k}: FAST and EXACT agree on this scene, the route would not show"
            if k in (0, 1, 2, 5):
                _assert_same(p[k], xp, f"world {k} (clamp {clamp[k]}) carries its EXACT positions")
                _assert_same(v[k], xv, f"world {k} (clamp {clamp[k]}) carries its EXACT velocities")
            else:
                _assert_same(p[k], fp, f"world {k} (clamp {clamp[k]}) carries its FAST positions")
                _assert_same(v[k], fv, f"world {k} (clamp {clamp[k]}) carries its FAST velocities")
            if k in (0, 3):
                op, ov, _ = orc.update_direct(pos[k], vel[k], w[k], delta=DELTA[k], clamp=clamp[k], nsteps=int(steps[k]), nthreads=NTH)
                assert _same(p[k], op) == (k == 0) and _same(v[k], ov) == (k == 0), k


# ------------------------------------------------------------------ 6. tracers
TB = 5                                            # worlds of the tracer cases
TSTEPS = np.array([2, 0, 1, 2, 1], np.int32)


def _tracers(n, m, dtype):
    """m tracers per world in the bodies' box; tracer 0 of every world sits 2^-11 from body 0 (under every clamp)."""
    t = np.dtype(dtype).type
    pos = _scene(n, dtype, TB)[0]
    rng = np.random.default_rng(9000 + n + m)
    tp = (rng.random((TB, m, 2)) * 4 + 1).astype(t)
    tp[:, 0] = pos[:, 0] + np.array([0, PAIR / 2], t)
    tv = (rng.standard_normal((TB, m, 2)) * 0.1).astype(t)
    return tp, tv


def _euler(tp, tv, acc, dt):
    """main.rs:419-423 in the arrays' dtype, multiply then add."""
    t = tp.dtype.type
    v = tv + acc.astype(t) * t(dt)
    return tp + v * t(dt), v


def _oracle_tracers(orc, pos, vel, w, tp, tv, delta, clamp, steps):
    """Tracers by direct_accel at the pre-step bodies + Euler, bodies by update_direct, step by step -> (tp, tv)."""
    t = pos.dtype.type
    for _ in range(int(steps)):
        acc = orc.direct_accel(pos, w, target_pos=tp, clamp=clamp, accum="native", nthreads=NTH)[0]
        tp, tv = _euler(tp, tv, acc, t(delta))
        pos, vel, _ = orc.update_direct(pos, vel, w, delta=delta, clamp=clamp, nsteps=1, nthreads=NTH)
    return tp, tv


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("arith", ["exact", "fast", "auto"])
@pytest.mark.parametrize("m", [1, 511, 512, 513])
@pytest.mark.parametrize("n", [3, 129])
def test_tracers_follow_their_worlds_parameters(nb, orc, n, m, arith, dtype):
    pos, vel, w = _scene(n, dtype, TB)
    tp, tv = _tracers(n, m, dtype)
    delta, clamp = DELTA[:TB], CLAMP[:TB]
    _scene_is_telling(orc, pos, vel, w, delta, clamp, key=(n, dtype, TB))
    cls = _cls(nb, dtype, "RestrictedEnsemble")
    with cls(pos, vel, w, (tp, tv), arith=arith, clamp=0.5) as r:
        r.sweep(delta, clamp, TSTEPS)
        p, v, _ = r.particles()
        gp, gv = r.tracers()
    _assert_same(gp[1], tp[1], "tracer positions of the world of 0 steps")
    _assert_same(gv[1], tv[1], "tracer velocities of the world of 0 steps")
    assert not _same(gp[0], tp[0])
    if arith == "exact":
        for k in range(TB):
            rtp, rtv = _oracle_tracers(orc, pos[k], vel[k], w[k], tp[k], tv[k], delta[k], clamp[k], TSTEPS[k])
            _assert_same(gp[k], rtp, f"tracer positions of world {k}")
            _assert_same(gv[k], rtv, f"tracer velocities of world {k}")
            # one oracle step under the neighbour's clamp moves tracer 0 elsewhere: the clamp that was applied is the world's
            if TSTEPS[k] == 1:
                other = _oracle_tracers(orc, pos[k], vel[k], w[k], tp[k], tv[k], delta[k], clamp[(k + 1) % TB], 1)
                assert not _same(other[1][0], rtv[0]), k
        return
    with cls(pos[:1], vel[:1], w[:1], (tp[:1], tv[:1]), arith=arith) as single:
        for k in range(TB):
            single.upload(pos[k:k + 1], vel[k:k + 1], w[k:k + 1], (tp[k:k + 1], tv[k:k + 1]))
            single.h.set_params(clamp=float(clamp[k]))
            single.update(float(delta[k]), None, n_steps=int(TSTEPS[k]))
            ap, av, _ = single.particles()
            atp, atv = single.tracers()
            _assert_same(p[k], ap[0], f"{arith}: positions of world {k}")
            _assert_same(v[k], av[0], f"{arith}: velocities of world {k}")
            _assert_same(gp[k], atp[0], f"{arith}: tracer positions of world {k}")
            _assert_same(gv[k], atv[0], f"{arith}: tracer velocities of world {k}")


@pytest.mark.parametrize("dtype,arith,tiny", [("float32", "auto", 1e-8), ("float64", "fast", 1e-305)])
def test_a_tracer_outside_fasts_domain_takes_its_exact_value_in_a_fast_world(nb, orc, dtype, arith, tiny):
    """World 2 takes one step under a clamp FAST accepts, with every body inside FAST's domain: a FAST world.  Its tracer 5 sits
    at (tiny, tiny), outside the domain: it gets the oracle's value; its neighbour, tracer 4, keeps FAST bits."""
    n, m, k = 129, 513, 2
    pos, vel, w = _scene(n, dtype, TB)
    tp, tv = _tracers(n, m, dtype)
    tp[k, 5] = [tiny, tiny]
    delta, clamp = DELTA[:TB], CLAMP[:TB]
    assert TSTEPS[k] == 1 and clamp[k] >= FLOOR
    cls = _cls(nb, dtype, "RestrictedEnsemble")
    with cls(pos, vel, w, (tp, tv), arith=arith) as r:
        r.sweep(delta, clamp, TSTEPS)
        gp, gv = r.tracers()
    rtp, rtv = _oracle_tracers(orc, pos[k], vel[k], w[k], tp[k], tv[k], delta[k], clamp[k], 1)
    _assert_same(gp[k, 5], rtp[5], "the tracer outside the domain: its EXACT position")
    _assert_same(gv[k, 5], rtv[5], "the tracer outside the domain: its EXACT velocity")
    assert not _same(gv[k, 4], rtv[4]), "its neighbour carries FAST bits"
    assert not _same(gv[k], rtv)


# ------------------------------------------------------------------ 7. ragged and ragged restricted, both precisions
RSIZES = [5, 128, 129, 600, 2049, 64]             # four launch classes: <= 128, <= 256, <= 1024, <= 4096
RCOUNTS = [0, 1, 513, 2, 600, 3]
RSTEPS = np.array([2, 1, 3, 0, 2, 3], np.int32)


def _ragged_worlds(dtype):
    t = np.dtype(dtype).type
    worlds = [_world(n, 9500 + k, t) for k, n in enumerate(RSIZES)]
    rng = np.random.default_rng(9600)
    tracers = []
    for k, m in enumerate(RCOUNTS):
        if not m:
            tracers.append(None)
            continue
        tp = (rng.random((m, 2)) * 4 + 1).astype(t)
        tp[0] = worlds[k][0][0] + np.array([0, PAIR / 2], t)
        tracers.append((tp, (rng.standard_normal((m, 2)) * 0.1).astype(t)))
    return worlds, tracers


def _run_ragged(cls, worlds, tracers, arith, delta, clamp, steps, order):
    ps, vs, ws = ([worlds[k][i] for k in order] for i in range(3))
    kw = {} if tracers is None else dict(tracers=[tracers[k] for k in order])
    with cls(ps, vs, ws, arith=arith, clamp=0.5, **kw) as e:
        e.sweep(delta[order], clamp[order], steps[order])
        p, v, _ = e.particles()
        return p, v, (e.tracers() if tracers is not None else None)


@pytest.mark.parametrize("arith", ["exact", "fast", "auto"])
@pytest.mark.parametrize("kind", ["RaggedEnsemble", "RaggedEnsemble64", "RaggedRestrictedEnsemble", "RaggedRestrictedEnsemble64"])
def test_ragged_worlds_are_the_worlds_alone_and_parameters_follow_the_world(nb, orc, kind, arith):
    dtype = "float64" if kind.endswith("64") else "float32"
    worlds, tracers = _ragged_worlds(dtype)
    if "Restricted" not in kind:
        tracers = None
    if arith == "exact":    # (once per precision: the scene tells the parameters apart)
        _scene_is_telling(orc, [x[0] for x in worlds], [x[1] for x in worlds], [x[2] for x in worlds], DELTA, CLAMP, key=("ragged", dtype))
    cls = getattr(nb, kind)
    order = np.arange(B)
    p, v, tr = _run_ragged(cls, worlds, tracers, arith, DELTA, CLAMP, RSTEPS, order)
    for k in range(B):
        kw = {} if tracers is None else dict(tracers=[tracers[k]])
        with cls([worlds[k][0]], [worlds[k][1]], [worlds[k][2]], arith=arith, clamp=float(CLAMP[k]), **kw) as single:
            single.update(float(DELTA[k]), None, n_steps=int(RSTEPS[k]))
            ap, av, _ = single.particles()
            _assert_same(p[k], ap[0], f"{arith}: positions of world {k}")
            _assert_same(v[k], av[0], f"{arith}: velocities of world {k}")
            if tracers is not None:
                (atp, atv), = single.tracers()
                _assert_same(tr[k][0], atp, f"{arith}: tracer positions of world {k}")
                _assert_same(tr[k][1], atv, f"{arith}: tracer velocities of world {k}")
    _assert_same(p[3], worlds[3][0], "the world of 0 steps")
    # the worlds in reversed order with reversed arrays: the reversed results (the parameters follow the world, not the item)
    rev = order[::-1].copy()
    qp, qv, qtr = _run_ragged(cls, worlds, tracers, arith, DELTA, CLAMP, RSTEPS, rev)
    for i, k in enumerate(rev):
        _assert_same(qp[i], p[k], f"{arith}: reversed upload, positions of world {k}")
        _assert_same(qv[i], v[k], f"{arith}: reversed upload, velocities of world {k}")
        if tracers is not None:
            _assert_same(qtr[i][0], tr[k][0], f"{arith}: reversed upload, tracer positions of world {k}")
            _assert_same(qtr[i][1], tr[k][1], f"{arith}: reversed upload, tracer velocities of world {k}")


# ------------------------------------------------------------------ 8. with the hand-offs
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_delta_streams_frames_and_split_calls_after_a_sweep(nb, orc, dtype):
    n = 65
    pos, vel, w = _scene(n, dtype)
    steps, n_steps = _steps_for(n)
    cls = _cls(nb, dtype)
    with cls(pos, vel, w, arith="auto") as e, cls(pos, vel, w, arith="auto") as split:
        dec = nb.DeltasDecoder(B)
        streams, step0 = e.deltas()
        dec.apply(streams)
        e.update(0.1, None, n_steps=2)
        e.upload(pos, vel, w)                                  # (the count runs on across uploads)
        streams, step1 = e.deltas()
        dec.apply(streams)
        assert (step0, step1) == (0, 2)
        e.sweep(DELTA, CLAMP, steps)
        p, v, _ = e.particles()
        streams, step2 = e.deltas()
        assert step2 == step1 + n_steps                        # the handle's launches, not any world's own steps
        for k, s in enumerate(streams):
            assert int.from_bytes(s[16:24], "little") == step2, k
        dec.apply(streams)
        for k, got in enumerate(dec.positions()):
            _assert_same(got, p[k], f"decoded positions of world {k}")
        dec.close()
        frames = e.frames(height=8, render_px=8)
        for k in range(B):
            assert np.array_equal(frames[k], orc.draw(p[k], v[k], w[k], 8, 8)), k
        assert len({frames[k].tobytes() for k in range(B)}) > 1
        # one sweep split into two calls, the steps split accordingly
        first = np.minimum(steps, 1).astype(np.int32)
        split.sweep(DELTA, CLAMP, first, n_steps=1)
        split.sweep(DELTA, CLAMP, steps - first, n_steps=n_steps - 1)
        sp, sv, _ = split.particles()
    _assert_same(sp, p, "positions of the split sweep")
    _assert_same(sv, v, "velocities of the split sweep")


# ------------------------------------------------------------------ 9. refusals
WORDS = {"Ensemble": "ensemble", "RaggedEnsemble": "ragged", "RestrictedEnsemble": "restricted", "RaggedRestrictedEnsemble": "ragged restricted"}


@pytest.mark.parametrize("kind", ["Ensemble", "Ensemble64", "RaggedEnsemble", "RaggedEnsemble64", "RestrictedEnsemble",
                                  "RestrictedEnsemble64", "RaggedRestrictedEnsemble", "RaggedRestrictedEnsemble64"])
def test_refusals_name_the_handle_and_sweep_and_leave_it_working(nb, kind):
    """The library's own refusals (the Python method checks the same things first, so the handle's call is used here)."""
    C = nb._capi
    dtype = "float64" if kind.endswith("64") else "float32"
    word = WORDS[kind[:-2] if kind.endswith("64") else kind]
    pos, vel, w = _scene(65, dtype)
    cls = getattr(nb, kind)
    ragged = kind.startswith("Ragged")
    make = (lambda: cls(list(pos), list(vel), list(w), arith="auto")) if ragged else (lambda: cls(pos, vel, w, arith="auto"))
    delta = np.ascontiguousarray(DELTA, dtype=dtype)
    steps = np.array([1, 2, 0, 2, 1, 2], np.int32)

    def refused(h, what, *args):
        with pytest.raises(C.NBodyError) as err:
            h.sweep(*args)
        assert err.value.code == C.ERR_INVALID
        msg = str(err.value)
        assert msg[msg.index(word):].startswith(word + " sweep") and what in msg, msg

    fresh = type(make().h)(0)                                   # a handle of this kind with nothing uploaded
    try:
        refused(fresh, "nothing uploaded", delta, CLAMP, steps, 2)
    finally:
        fresh.close()
    with make() as e, make() as want:
        refused(e.h, "delta", None, CLAMP, steps, 2)
        refused(e.h, "n_steps", delta, CLAMP, steps, -1)
        bad = steps.copy()
        bad[3] = 3
        refused(e.h, "world 3", delta, CLAMP, bad, 2)
        bad[3] = -1
        refused(e.h, "world 3", delta, CLAMP, bad, 2)
        refused(e.h, "world 0", delta, CLAMP, steps, 0)         # (the checks come before the no-op)
        e.h.sweep(delta, CLAMP, np.zeros(B, np.int32), 0)       # n_steps == 0 after the checks: a no-op
        e.h.sweep(delta, None, None, 0)
        p0 = e.particles()
        _assert_same(np.concatenate(p0[0]) if ragged else p0[0], np.concatenate(list(pos)) if ragged else pos, "n_steps == 0")
        e.sweep(DELTA, CLAMP, steps)                            # and the handle works
        want.sweep(DELTA, CLAMP, steps)
        (p, v, _), (wp, wv, _) = e.particles(), want.particles()
        for k in range(B):
            _assert_same(p[k], wp[k], f"positions of world {k} after the refusals")
            _assert_same(v[k], wv[k], f"velocities of world {k} after the refusals")
        assert not _same(p[0], pos[0]) and _same(p[2], pos[2])
