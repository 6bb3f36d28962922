"""Tracers (nbody_tracers_*, Context.upload_tracers, World(tracers=...)): points without mass that step with the bodies on the
device, against the CPU oracle.

EXACT direct steps are bit-identical to two independent constructions (the oracle's update_direct with the tracers as weight-0
bodies; the oracle's direct_accel at the tracers + Euler in numpy); tree steps to the oracle's walk at the tracers + Euler; FAST is
within the project's frozen tolerances (tests/_tol.py ACC_RTOL for f32, 1e-12 of sum |term| for f64); the bodies' rows never
notice the tracers; a tracer's rows depend on its own state and the bodies alone.  Needs an MI355X."""
import numpy as np
import pytest

from _tol import check_fast
from test_gpu_direct_probes import _targets

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
FAST64_RTOL = 1e-12
NTH = 16
DT = 0.1


@pytest.fixture(scope="module")
def ctx(nb):
    c = nb._capi.Context(0)
    yield c
    c.close()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))  # bit for bit, whatever the dtype (floats, ids, pixels)


def _set(ctx, C, arith, **kw):
    ctx.set_params(arith={"auto": C.ARITH_AUTO, "fast": C.ARITH_FAST, "exact": C.ARITH_EXACT}[arith], **kw)


def _euler(p, v, a, dt):
    """main.rs:419-423 in the arrays' dtype: v += a*dt; x += v*dt, multiply then add (numpy rounds every operation)."""
    d = p.dtype.type(dt)
    with np.errstate(all="ignore"):
        v = v + a.astype(p.dtype) * d
        p = p + v * d
    return p, v


def _tracer_set(rng, pos, dt, m, clamp=0.001, with_skip=True):
    """m tracers: points on bodies, at 0.5 sqrt(clamp) from bodies and random ones (all finite), and — m allowing, for the direct
    sum — the skip cases behind them -> (pos, vel, number of finite ones in front)."""
    fin, skip = _targets(rng, pos, clamp, dt, n_random=max(m, 4), n_on=64, n_near=64)
    fin = np.concatenate([fin[-128:-64][:1], fin[-64:][:1], fin[:-128][:2], fin[-128:], fin[:-128][2:]])  # on, near, random first
    if with_skip and m > 2 * len(skip):
        tp = np.concatenate([fin[:m - len(skip)], skip])
        n_fin = m - len(skip)
    else:
        tp, n_fin = fin[:m], m
    tv = rng.normal(0, 1, tp.shape).astype(dt)
    return np.ascontiguousarray(tp), tv, n_fin


def _ref_b_direct(orc, pos, vel, w, tp, tv, steps, clamp=0.001):
    """Reference (b): the bodies alone by the oracle's step; the tracers by direct_accel at the pre-step bodies + Euler."""
    for _ in range(steps):
        a, _n = orc.direct_accel(pos, w, target_pos=tp, clamp=clamp, accum="native", nthreads=NTH)
        tp, tv = _euler(tp, tv, a, DT)
        pos, vel, _c = orc.update_direct(pos, vel, w, delta=DT, clamp=clamp, nsteps=1, nthreads=NTH)
    return pos, vel, tp, tv


# ---- 1. EXACT direct, bit for bit, two independent references
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("n", [1, 63, 1024, 65537])
@pytest.mark.parametrize("m", [1, 300, 70000])
def test_exact_direct_steps_equal_both_references_bit_for_bit(nb, orc, ctx, dt, n, m):
    C = nb._capi
    pos, vel, w = nb.scenes.plummer(n, seed=0x7A + n, dtype=dt)
    if n >= 1024:
        w = np.random.default_rng(n).integers(1, 1000, n).astype(np.uint32)
    rng = np.random.default_rng(1000 * n + m)
    tp, tv, n_fin = _tracer_set(rng, pos, dt, m)
    _set(ctx, C, "exact")
    ctx.upload(pos, vel, w)
    ctx.upload_tracers(tp, tv)
    assert ctx.n_tracers == m
    ctx.update_direct(DT, 3)
    p, v, _, _ = ctx.download()
    gp, gv = ctx.download_tracers()
    assert gp.dtype == dt and gp.shape == (m, 2)
    # (b) every tracer, skip cases included
    rp, rv, rtp, rtv = _ref_b_direct(orc, pos, vel, w, tp, tv, 3)
    assert _same(p, rp) and _same(v, rv)
    assert _same(gp, rtp) and _same(gv, rtv)
    # (a) the finite tracers as weight-0 bodies behind the bodies
    ap, av, _c = orc.update_direct(np.concatenate([pos, tp[:n_fin]]), np.concatenate([vel, tv[:n_fin]]),
                                   np.concatenate([w, np.zeros(n_fin, np.uint32)]), delta=DT, nsteps=3, nthreads=NTH)
    assert _same(p, ap[:n]) and _same(v, av[:n])
    assert _same(gp[:n_fin], ap[n:]) and _same(gv[:n_fin], av[n:])


# ---- 2. the bodies never notice
def _bodies_after(ctx, C, pos, vel, w, tracers, step):
    ctx.upload(pos, vel, w)
    if tracers is not None:
        ctx.upload_tracers(*tracers)
    step()
    return ctx.download()


@pytest.mark.parametrize("case", ["f32_auto_small", "f32_fast_small", "f32_exact_small", "f32_auto_classes", "f32_fast_classes",
                                  "f32_exact_classes", "f64_auto", "f64_fast", "bvh_f32", "bvh_f64", "bvh_f32_consistent",
                                  "bvh_f64_consistent", "quad_f32", "quad_f64"])
def test_bodies_are_bit_identical_with_and_without_tracers(nb, ctx, case):
    C = nb._capi
    dt = F64 if "f64" in case else F32
    rng = np.random.default_rng(7)
    if case.startswith(("bvh", "quad")):
        n = 20000
        pos, vel, _ = nb.scenes.plummer(n, seed=0x2B, dtype=dt)
        w = rng.integers(1, 100, n).astype(np.uint32)
        kind = C.TREE_BVH if case.startswith("bvh") else C.TREE_QUAD
        _set(ctx, C, "auto", theta=0.5, leaf_size=64, order=C.ORDER_CONSISTENT if "consistent" in case else C.ORDER_AS_WRITTEN)
        step = lambda: ctx.update_tree(kind, DT, 6)  # noqa: E731  (six: BVH steps without tracers are enqueued ahead)
    else:
        n = 32768 if "classes" in case else (4096 if dt == F32 else 8192)
        pos, vel, w = nb.scenes.plummer(n, seed=0x2C, dtype=dt)
        if "classes" in case:
            w = (np.arange(n) % 5 + 1).astype(np.uint32)
        _set(ctx, C, case.split("_")[1])
        step = lambda: ctx.update_direct(DT, 6)  # noqa: E731  (six: a small f32 step without tracers replays a captured graph)
    tp, tv, _ = _tracer_set(rng, pos, dt, 5000, with_skip=not case.startswith(("bvh", "quad")))
    plain = _bodies_after(ctx, C, pos, vel, w, None, step)
    with_tr = _bodies_after(ctx, C, pos, vel, w, (tp, tv), step)
    for a, b in zip(plain, with_tr):
        assert _same(a, b)
    gp, _ = ctx.download_tracers()
    assert not _same(gp, tp)  # (and the tracers did move)
    _set(ctx, C, "auto", theta=50.0, order=C.ORDER_AS_WRITTEN)


# ---- 3. trees
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("theta", [0.5, 50.0])
@pytest.mark.parametrize("kind", ["bvh", "quad"])
def test_tree_steps_equal_the_oracles_walk_at_the_tracers(nb, orc, ctx, dt, theta, kind):
    C = nb._capi
    n, m = 20000, 5000
    pos, vel, _ = nb.scenes.plummer(n, seed=0x3E, dtype=dt)
    rng = np.random.default_rng(11)
    w = rng.integers(1, 100, n).astype(np.uint32)
    tp, tv, _ = _tracer_set(rng, pos, dt, m, with_skip=False)
    _set(ctx, C, "auto", theta=theta, leaf_size=64, order=C.ORDER_AS_WRITTEN)
    ctx.upload(pos, vel, w)
    ctx.upload_tracers(tp, tv)
    ctx.update_tree(C.TREE_BVH if kind == "bvh" else C.TREE_QUAD, DT, 3)
    rp, rv, rw, rids = pos, vel, w, None
    for _ in range(3):
        tree = orc.BVH(rp, rw, leaf_size=64) if kind == "bvh" else orc.Quad(rp, rw)
        a = tree.walk(tp, theta=theta, nthreads=NTH)
        tree.close()
        tp, tv = _euler(tp, tv, a, DT)
        if kind == "bvh":
            rp, rv, rw, rids, _c = orc.update_bvh(rp, rv, rw, delta=DT, theta=theta, leaf_size=64, mode=orc.AS_WRITTEN, nsteps=1,
                                                  nthreads=NTH, ids=rids)
        else:
            rp, rv, _c = orc.update_quad(rp, rv, rw, delta=DT, theta=theta, nsteps=1, nthreads=NTH)
    p, v, w2, ids = ctx.download()
    assert _same(p, rp) and _same(v, rv) and np.array_equal(w2, rw)
    gp, gv = ctx.download_tracers()
    assert _same(gp, tp) and _same(gv, tv)
    _set(ctx, C, "auto", theta=50.0)


@pytest.mark.parametrize("dt", [F32, F64])
def test_direct_and_tree_steps_interleave_with_tracers(nb, orc, ctx, dt):
    C = nb._capi
    pos, vel, _ = nb.scenes.plummer(2048, seed=0xD6409, dtype=dt)
    w = (np.arange(2048) % 7 + 1).astype(np.uint32)
    rng = np.random.default_rng(13)
    tp, tv, _ = _tracer_set(rng, pos, dt, 700, with_skip=False)
    _set(ctx, C, "exact", theta=0.5, leaf_size=64, order=C.ORDER_AS_WRITTEN)
    ctx.upload(pos, vel, w)
    ctx.upload_tracers(tp, tv)
    ctx.update_direct(DT, 2)
    ctx.update_tree(C.TREE_BVH, DT, 1)
    ctx.update_direct(DT, 1)
    ctx.update_tree(C.TREE_QUAD, DT, 2)
    ctx.update_direct(DT, 1)
    rp, rv, rw, rids = pos, vel, w, None
    for what in ("direct", "direct", "bvh", "direct", "quad", "quad", "direct"):
        if what == "direct":
            a, _n = orc.direct_accel(rp, rw, target_pos=tp, accum="native", nthreads=NTH)
            nrp, nrv, _c = orc.update_direct(rp, rv, rw, delta=DT, nsteps=1, nthreads=NTH)
        elif what == "bvh":
            tree = orc.BVH(rp, rw, leaf_size=64)
            a = tree.walk(tp, theta=0.5, nthreads=NTH)
            tree.close()
            nrp, nrv, rw, rids, _c = orc.update_bvh(rp, rv, rw, delta=DT, theta=0.5, mode=orc.AS_WRITTEN, nsteps=1, nthreads=NTH, ids=rids)
        else:
            tree = orc.Quad(rp, rw)
            a = tree.walk(tp, theta=0.5, nthreads=NTH)
            tree.close()
            nrp, nrv, _c = orc.update_quad(rp, rv, rw, delta=DT, theta=0.5, nsteps=1, nthreads=NTH)
        tp, tv = _euler(tp, tv, a, DT)
        rp, rv = nrp, nrv
    p, v, w2, ids = ctx.download()
    assert np.array_equal(ids, rids) and np.array_equal(w2, rw)
    assert _same(p, rp) and _same(v, rv)
    gp, gv = ctx.download_tracers()
    assert _same(gp, tp) and _same(gv, tv)
    _set(ctx, C, "auto", theta=50.0)


# ---- 4. FAST through the public step: velocity 0, delta 1, one step — the downloaded velocity is the acceleration
def _accel_through_a_step(ctx, bodies, tp):
    ctx.upload(*bodies)  # (the step moves the bodies: every measurement starts from the same ones)
    ctx.upload_tracers(tp, np.zeros_like(tp))
    ctx.update_direct(1.0, 1)
    return ctx.download_tracers()[1]


@pytest.mark.parametrize("case", ["plummer", "free_masses", "reference_scene"])
def test_fast_f32_steps_within_tolerance(nb, orc, ctx, case):
    C = nb._capi
    rng = np.random.default_rng(23)
    if case == "reference_scene":
        pos, vel, w = nb.scenes.galaxy()
        tp, _ = _targets(rng, pos, 0.001, F32, n_random=8192)
        heavy = pos[:2].astype(F64)
        tp = np.concatenate([tp, (heavy + 0.5 * np.sqrt(0.001)).astype(F32), (heavy + 3.0).astype(F32)])
    else:
        pos, vel, w = nb.scenes.plummer(65536, seed=0xFA57, dtype=F32)
        if case == "free_masses":
            w = nb.scenes.free_weights(65536)
        tp = np.concatenate([pos[:4096], _targets(rng, pos, 0.001, F32, n_random=4096)[0]])
    ref64, norm = orc.direct_accel(pos, w, target_pos=tp, accum="f64", nthreads=NTH)
    for arith in ("fast", "auto"):
        _set(ctx, C, arith)
        acc = _accel_through_a_step(ctx, (pos, vel, w), tp)
        check_fast(acc, ref64, norm)
    ex, _n = orc.direct_accel(pos, w, target_pos=tp[:512], accum="native", nthreads=NTH)
    assert not _same(acc[:512], ex.astype(F32))  # FAST really ran


def test_fast_f64_steps_within_1e_12(nb, orc, ctx):
    C = nb._capi
    pos, vel, _ = nb.scenes.plummer(65536, seed=0xF64, dtype=F64)
    w = np.random.default_rng(31).integers(1, 1000, 65536).astype(np.uint32)
    rng = np.random.default_rng(37)
    tp = (pos[:8192] + rng.normal(0, 2, (8192, 2))).astype(F64)
    tp[:128] = pos[1000:1128]  # some on bodies
    _set(ctx, C, "fast")
    acc = _accel_through_a_step(ctx, (pos, vel, w), tp)
    ref, norm = orc.direct_accel(pos, w, target_pos=tp, accum="f64", nthreads=NTH)
    err = np.abs(acc - ref).sum(axis=1) / np.maximum(norm, 1e-300)
    assert np.all(np.isfinite(err)) and err.max() <= FAST64_RTOL, err.max()
    ex, _n = orc.direct_accel(pos, w, target_pos=tp[:512], accum="native", nthreads=NTH)
    assert not _same(acc[:512], ex)
    # a tracer outside the f64 FAST domain takes its EXACT value, the others keep their FAST bits
    bad = np.array([[2.0 ** 101, 0.0], [1e-305, 1.0]])
    mixed = _accel_through_a_step(ctx, (pos, vel, w), np.concatenate([tp[:1000], bad]))
    bx, _n = orc.direct_accel(pos, w, target_pos=bad, accum="native", nthreads=NTH)
    assert _same(mixed[:1000], acc[:1000]) and _same(mixed[1000:], bx)


def test_auto_f32_a_tracer_outside_the_domain_takes_its_exact_value(nb, orc, ctx):
    C = nb._capi
    pos, vel, w = nb.scenes.plummer(65536, seed=0xA070, dtype=F32)
    rng = np.random.default_rng(47)
    fin = _targets(rng, pos, 0.001, F32, n_random=2000)[0]
    bad = np.array([[2.0 ** 61, 3.0], [1e-39, 7.0]], F32)
    _set(ctx, C, "auto")
    plain = _accel_through_a_step(ctx, (pos, vel, w), fin)
    mixed = _accel_through_a_step(ctx, (pos, vel, w), np.concatenate([fin[:700], bad[:1], fin[700:1500], bad[1:], fin[1500:]]))
    assert _same(np.concatenate([mixed[:700], mixed[701:1501], mixed[1502:]]), plain)
    ex, _n = orc.direct_accel(pos, w, target_pos=bad, accum="native", nthreads=NTH)
    assert _same(mixed[[700, 1501]], ex.astype(F32))
    fx, _n = orc.direct_accel(pos, w, target_pos=fin, accum="native", nthreads=NTH)
    assert not _same(plain, fx.astype(F32))  # the finite ones ran FAST


def test_auto_f32_a_nan_body_makes_every_tracer_exact(nb, orc, ctx):
    C = nb._capi
    pos, vel, w = nb.scenes.plummer(65536, seed=0xA071, dtype=F32)
    pos[1234] = (np.nan, 5.0)
    tp = _targets(np.random.default_rng(53), pos, 0.001, F32, n_random=1000)[0]
    _set(ctx, C, "auto")
    ex, _n = orc.direct_accel(pos, w, target_pos=tp, accum="native", nthreads=NTH)
    assert _same(_accel_through_a_step(ctx, (pos, vel, w), tp), ex.astype(F32))


# ---- 4b. a step that carries a tracer across the boundary of FAST's domain integrates it once
def _outside_fast(p):
    """FAST's domain per coordinate (include/nbody_hip.h): f32 below 2^60, f64 below 2^100, in magnitude; zero or at least 2^-22 /
    2^-300; finite."""
    big, tiny = (2.0 ** 60, 2.0 ** -22) if p.dtype == F32 else (2.0 ** 100, 2.0 ** -300)
    a = np.abs(p.astype(F64))
    return np.any(~(a < big) | ((a != 0) & (a < tiny)), axis=1)


def _crossing_tracers(dt):
    """(pos, vel) of tracers that one step of DT carries out of FAST's domain (rows 0-1: past its upper bound; f32 also the rows
    from 4 on: into (0, 2^-22)) and of tracers that start outside and come in (rows 2-3)."""
    e = 59 if dt == F32 else 99
    sub = 1e-39 if dt == F32 else 1e-305
    tp = [[1.5 * 2.0 ** e, 7.0], [3.0, -1.25 * 2.0 ** e], [2.0 ** (e + 2), 3.0], [sub, 7.0]]
    tv = [[2.0 ** (e + 4), 0.0], [0.0, -(2.0 ** (e + 4))], [-(2.0 ** (e + 5)), 0.0], [1.0, 0.0]]
    if dt == F32:  # a ladder of velocities around -1: x = 0.1 + v*dt lands every 2e-8 over +-1.6e-7 around zero, inside (-2^-22, 2^-22)
        for k in range(-8, 9):  # (wherever the bodies' pull, a*dt^2, shifts the ladder by less than 1e-7, rungs land there)
            tp.append([0.1, 60000.0 + k])
            tv.append([-1.0 + 2e-7 * k, 0.0])
    return np.array(tp, dt), np.array(tv, dt)


@pytest.mark.parametrize("dt,arith", [(F32, "auto"), (F64, "fast")])
def test_a_tracer_that_crosses_the_domain_boundary_is_integrated_once(nb, orc, ctx, dt, arith):
    """The route of a tracer in a step is decided once, from its pre-step position.  Reference: the same arithmetic through the
    probe call — Context.accel_direct(tracers) on the pre-step bodies — + Euler in numpy, the bodies stepped without tracers; a
    tracer's bits are the same through either door (per-target determinism), so the rows must agree bit for bit over several steps.
    The tracers that are EXACT in a step are also checked against the oracle's direct_accel for that step."""
    C = nb._capi
    n = 20000
    pos, vel, _ = nb.scenes.plummer(n, seed=0xC055, dtype=dt)
    w = np.random.default_rng(83).integers(1, 1000, n).astype(np.uint32)
    rng = np.random.default_rng(89)
    fp, fv, _ = _tracer_set(rng, pos, dt, 2000, with_skip=False)
    xp, xv = _crossing_tracers(dt)
    tp, tv = np.concatenate([fp[:1000], xp, fp[1000:]]), np.concatenate([fv[:1000], xv, fv[1000:]])
    _set(ctx, C, arith)
    steps = 3
    ctx.upload(pos, vel, w)
    ctx.upload_tracers(tp, tv)
    ctx.update_direct(DT, steps)
    gp, gv = ctx.download_tracers()
    bodies_with = ctx.download()
    ctx.upload(pos, vel, w)  # the reference run: no tracers
    rp, rv = tp, tv
    went_out = came_in = 0
    for _ in range(steps):
        bp = ctx.download()[0]
        a = ctx.accel_direct(rp)
        out_before = _outside_fast(rp)
        ex, _n = orc.direct_accel(bp, w, target_pos=rp[out_before], accum="native", nthreads=NTH)
        assert _same(a[out_before], ex.astype(dt))  # (outside the domain: the EXACT chain)
        rp, rv = _euler(rp, rv, a, DT)
        out_after = _outside_fast(rp)
        went_out += int(np.sum(~out_before & out_after))
        came_in += int(np.sum(out_before & ~out_after))
        ctx.update_direct(DT, 1)
    assert went_out >= (3 if dt == F32 else 2) and came_in >= 2, (went_out, came_in)  # the cases this test is about did occur
    assert _same(gp, rp) and _same(gv, rv)
    for x, y in zip(bodies_with, ctx.download()):
        assert _same(x, y)


# ---- 5. independence and determinism
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("arith", ["fast", "exact", "auto"])
def test_a_tracer_depends_on_its_own_state_and_the_bodies_alone(nb, ctx, dt, arith):
    C = nb._capi
    n = 20000
    pos, vel, _ = nb.scenes.plummer(n, seed=0xDE7, dtype=dt)
    w = np.random.default_rng(41).integers(1, 1000, n).astype(np.uint32)
    rng = np.random.default_rng(43)
    tp, tv, _ = _tracer_set(rng, pos, dt, 3000)  # (the skip cases at its end lie outside FAST's domain: the fix-up pass under AUTO)
    xp, xv = _crossing_tracers(dt)
    tp, tv = np.concatenate([tp[:1500], xp, tp[1500:]]), np.concatenate([tv[:1500], xv, tv[1500:]])
    _set(ctx, C, arith)

    def run(p, v, calls=(3,)):
        ctx.upload(pos, vel, w)
        ctx.upload_tracers(p, v)
        for k in calls:
            ctx.update_direct(DT, k)
        return ctx.download_tracers()

    ref = run(tp, tv)
    again = run(tp, tv)
    assert _same(again[0], ref[0]) and _same(again[1], ref[1])  # two runs
    one = run(tp, tv, calls=(1, 1, 1))
    assert _same(one[0], ref[0]) and _same(one[1], ref[1])  # three calls of one step
    rev = run(tp[::-1], tv[::-1])
    assert _same(rev[0][::-1], ref[0]) and _same(rev[1][::-1], ref[1])
    for i in rng.choice(len(tp), 3, replace=False):
        alone = run(tp[i:i + 1], tv[i:i + 1])
        assert _same(alone[0], ref[0][i:i + 1]) and _same(alone[1], ref[1][i:i + 1]), i
    # 70 000 + 37 others first: the set off every batch, block and wave boundary it had alone
    k = 70037
    op = (rng.random((k, 2)) * 1e5).astype(dt)
    ov = rng.normal(0, 1, (k, 2)).astype(dt)
    big = run(np.concatenate([op, tp]), np.concatenate([ov, tv]))
    assert _same(big[0][k:], ref[0]) and _same(big[1][k:], ref[1])


# ---- 6. the restricted reference scene
def test_restricted_scene_equals_the_whole_scene_with_massless_light_bodies(nb, orc):
    pos, vel, w = nb.scenes.galaxy()
    (bp, bv, bw), (tp, tv) = nb.scenes.restricted(pos, vel, w, 2)
    world = nb.World(bp, bv, bw, method="direct", arith="exact", tracers=(tp, tv))
    try:
        world.update(DT, None, n_steps=5)
        p, v, _, _ = world.particles()
        gp, gv = world.tracers()
    finally:
        world.close()
    w0 = w.copy()
    w0[2:] = 0
    rp, rv, _c = orc.update_direct(pos, vel, w0, delta=DT, nsteps=5, nthreads=NTH)
    assert _same(p, rp[:2]) and _same(v, rv[:2])
    assert _same(gp, rp[2:]) and _same(gv, rv[2:])


# ---- 7. lifetime and refusals
def test_invalid_calls_name_tracers(nb, ctx):
    C = nb._capi
    lib = ctx.lib
    p32, p64 = np.ones((2, 2), F32), np.ones((2, 2), F64)
    up32, up64 = lib.nbody_tracers_upload_f32, lib.nbody_tracers_upload_f64
    dn32, dn64 = lib.nbody_tracers_download_f32, lib.nbody_tracers_download_f64

    def refused(rc, h):
        return rc == C.ERR_INVALID and b"tracers" in lib.nbody_last_error(h)

    fresh = C.Context(0)
    try:  # no particles
        assert refused(up32(fresh.h, 2, C._ptr(p32), C._ptr(p32)), fresh.h)
        assert refused(up64(fresh.h, 2, C._ptr(p64), C._ptr(p64)), fresh.h)
        assert lib.nbody_num_tracers(fresh.h) == 0
    finally:
        fresh.close()
    pos, vel, w = nb.scenes.plummer(256, seed=0xE, dtype=F32)
    _set(ctx, C, "auto")
    ctx.upload(pos, vel, w)
    assert refused(up32(ctx.h, -1, C._ptr(p32), C._ptr(p32)), ctx.h)
    assert refused(up32(ctx.h, 2, None, C._ptr(p32)), ctx.h)
    assert refused(up32(ctx.h, 2, C._ptr(p32), None), ctx.h)
    assert refused(up64(ctx.h, 2, C._ptr(p64), C._ptr(p64)), ctx.h)  # the other precision
    assert refused(dn64(ctx.h, C._ptr(p64), C._ptr(p64)), ctx.h)
    assert lib.nbody_num_tracers(ctx.h) == 0
    ctx.upload(pos.astype(F64), vel.astype(F64), w)
    assert refused(up32(ctx.h, 2, C._ptr(p32), C._ptr(p32)), ctx.h)
    assert up64(ctx.h, 2, C._ptr(p64), C._ptr(p64)) == C.OK and ctx.n_tracers == 2
    # calls that do not carry tracers
    assert refused(lib.nbody_update_tree_shard_f64(ctx.h, C.TREE_BVH, 0.1, 0, 128, None), ctx.h)
    assert refused(lib.nbody_export_slice_dev(ctx.h, 0, 1, None, None, None), ctx.h)
    assert refused(lib.nbody_import_rows_dev(ctx.h, 0, None, None, None), ctx.h)
    ctx.upload(pos, vel, w)
    ctx.upload_tracers(p32, p32)
    assert refused(lib.nbody_update_tree_async_f32(ctx.h, C.TREE_BVH, 0.1, 1), ctx.h)
    assert refused(lib.nbody_update_tree_shard_f32(ctx.h, C.TREE_BVH, 0.1, 0, 128, None), ctx.h)
    ctx.upload_tracers(np.zeros((0, 2), F32), np.zeros((0, 2), F32))  # m = 0 removes them, and the calls work again
    assert ctx.n_tracers == 0
    ctx.update_tree_async(C.TREE_BVH, 0.1, 1)
    ctx.wait()
    m = C.MultiContext([0], C.EXCHANGE_PEER)
    try:
        m.upload(pos, vel, w)
        assert refused(up32(m.h, 2, C._ptr(p32), C._ptr(p32)), m.h)
        assert refused(dn32(m.h, C._ptr(p32), C._ptr(p32)), m.h)
        assert lib.nbody_num_tracers(m.h) == 0
        with pytest.raises(C.NBodyError):
            m.upload_tracers(p32, p32)
    finally:
        m.close()


@pytest.mark.parametrize("dt", [F32, F64])
def test_lifetime_download_and_what_sees_bodies_only(nb, ctx, dt):
    C = nb._capi
    pos, vel, w = nb.scenes.plummer(3000, seed=0x11FE, dtype=dt)
    rng = np.random.default_rng(71)
    tp, tv, _ = _tracer_set(rng, pos, dt, 500, with_skip=False)
    _set(ctx, C, "auto", theta=0.5)
    lib = ctx.lib

    def outputs(tracers):
        ctx.upload(pos, vel, w)
        if tracers:
            ctx.upload_tracers(tp, tv)
        ctx.update_direct(DT, 0)  # n_steps == 0: a no-op
        ctx.update_tree(C.TREE_BVH, DT, 0)
        if tracers:
            gp, gv = ctx.download_tracers()
            assert _same(gp, tp) and _same(gv, tv)
        ctx.update_tree(C.TREE_BVH, DT, 2)
        ctx.update_direct(DT, 1)
        ctx.snapshot_begin()
        snap = ctx.snapshot_end()
        frame = ctx.render(100_000, 250)
        acc = ctx.accel_direct(tp[:64])
        if tracers:  # the parity hooks and the hand-offs left them alone
            assert ctx.n_tracers == len(tp)
        return snap[:4] + (frame, acc)

    a, b = outputs(False), outputs(True)
    for x, y in zip(a, b):
        assert _same(x, y)
    # download with NULL arrays: either, both
    gp, gv = ctx.download_tracers()
    only_p, only_v = np.zeros_like(gp), np.zeros_like(gv)
    dn = lib.nbody_tracers_download_f64 if dt == F64 else lib.nbody_tracers_download_f32
    assert dn(ctx.h, C._ptr(only_p), None) == C.OK and dn(ctx.h, None, C._ptr(only_v)) == C.OK and dn(ctx.h, None, None) == C.OK
    assert _same(only_p, gp) and _same(only_v, gv)
    # a new set replaces the old one; a body upload removes them
    ctx.upload_tracers(tp[:7], tv[:7])
    assert ctx.n_tracers == 7 and _same(ctx.download_tracers()[0], tp[:7])
    ctx.upload(pos, vel, w)
    assert ctx.n_tracers == 0 and ctx.download_tracers()[0].shape == (0, 2)
    _set(ctx, C, "auto", theta=50.0)


@pytest.mark.parametrize("method", ["direct_f32", "direct_f64", "bvh_f32"])
def test_the_timer_counts_the_bodies_kernel_only(nb, ctx, method):
    C = nb._capi
    dt = F64 if method.endswith("f64") else F32
    pos, vel, w = nb.scenes.plummer(8192, seed=0x71, dtype=dt)
    tp, tv, _ = _tracer_set(np.random.default_rng(73), pos, dt, 5000, with_skip=method.startswith("direct"))
    _set(ctx, C, "auto", theta=0.5)
    counts = []
    for tracers in (False, True):
        ctx.upload(pos, vel, w)
        if tracers:
            ctx.upload_tracers(tp, tv)
        t = C.Timer()
        try:
            ctx.set_timer(t)
            if method.startswith("direct"):
                ctx.update_direct(DT, 5)
            else:
                ctx.update_tree(C.TREE_BVH, DT, 5)
            counts.append(t.read()[1])
        finally:
            ctx.set_timer(None)
            t.close()
    # a direct step brackets one main pass: launches == n_steps.  A BVH walk may bracket more than one launch per step (a walk whose
    # estimate does not fit is launched again), so there the count is compared with the same steps without tracers.
    assert counts[0] == counts[1], counts
    if method.startswith("direct"):
        assert counts[1] == 5
    _set(ctx, C, "auto", theta=50.0)
