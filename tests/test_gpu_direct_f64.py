"""The direct O(N^2) step on an f64 context (nbody_update_direct_f64 / nbody_accel_direct_f64) against the CPU oracle.

EXACT and AUTO are bit-identical to the oracle's f64 direct sum and step; FAST is within 1e-12 of sum_j |term_ij|_1 per body
and falls back to the EXACT kernel, on the device, for a step with a position outside its domain.  Needs an MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F64 = np.float64
FAST_RTOL = 1e-12   # the FAST f64 contract


@pytest.fixture(scope="module")
def ctx(nb):
    c = nb._capi.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _fast_error(acc, ref, norm):
    err = np.abs(acc - ref).sum(axis=1)
    return err / np.maximum(norm, 1e-300)


def _uneven_weights(n, seed):
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 1000, n).astype(np.uint32)
    w[::5] = (1 << 24) + 1 + 2 * np.arange(len(w[::5]), dtype=np.uint32)   # past 2^24, odd: not exact in f32
    w[1::7] = np.uint32(0xFFFFFFFF) - np.arange(len(w[1::7]), dtype=np.uint32)  # near the u32 wrap
    return w


def _scene(nb, n, seed):
    pos, vel, _ = nb.scenes.plummer(n, seed=seed, dtype=F64)
    return pos, vel, _uneven_weights(n, seed)


def _set(ctx, C, arith, **kw):
    ctx.set_params(arith={"auto": C.ARITH_AUTO, "fast": C.ARITH_FAST, "exact": C.ARITH_EXACT}[arith], **kw)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1000, 4096])
@pytest.mark.parametrize("arith", ["exact", "auto"])
def test_accel_is_the_oracles_sum_bit_for_bit(nb, orc, ctx, n, arith):
    C = nb._capi
    pos, vel, w = _scene(nb, n, 0xD64 + n)
    _set(ctx, C, arith)
    ctx.upload(pos, vel, w)
    acc = ctx.accel_direct()
    ref, _ = orc.direct_accel(pos, w, accum="native", nthreads=8)
    assert acc.dtype == F64 and _same_bits(acc, ref)


def test_update_1024_bodies_10_steps(nb, orc, ctx):
    C = nb._capi
    pos, vel, w = _scene(nb, 1024, 0xD6401)
    _set(ctx, C, "exact")
    ctx.upload(pos, vel, w)
    cnt = C.Counting()
    ctx.update_direct(0.1, 10, cnt)
    p, v, w2, ids = ctx.download()
    rp, rv, _ = orc.update_direct(pos, vel, w, delta=0.1, nsteps=10, nthreads=8)
    assert _same_bits(p, rp) and _same_bits(v, rv)
    assert np.array_equal(w2, w) and np.array_equal(ids, np.arange(1024))
    assert cnt.sum_gravity > 0.0


def test_update_100_steps_on_the_ties_and_wraps_case(nb, orc, ctx):
    import os
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_inputs", "c_signs_ties_wrap")
    pos = np.fromfile(os.path.join(d, "pos0.f32"), "<f4").reshape(-1, 2).astype(F64)
    vel = np.fromfile(os.path.join(d, "vel0.f32"), "<f4").reshape(-1, 2).astype(F64)
    w = np.fromfile(os.path.join(d, "weight.u32"), "<u4")
    _set(ctx, nb._capi, "auto")
    ctx.upload(pos, vel, w)
    ctx.update_direct(0.1, 100)
    p, v, _, _ = ctx.download()
    rp, rv, _ = orc.update_direct(pos, vel, w, delta=0.1, nsteps=100, nthreads=8)
    assert _same_bits(p, rp) and _same_bits(v, rv)


def _skip_case(kind):
    """Bodies that exercise the is_normal skip (main.rs:241-243) in f64, among ordinary ones."""
    rng = np.random.default_rng(7)
    base = rng.uniform(-100.0, 100.0, (30, 2))
    tiny = np.ldexp(1.0, -1022)
    extra = {
        "coincident": [(5.0, 5.0), (5.0, 5.0), (5.0, 5.0)],
        "subnormal": [(0.0, 0.0), (np.ldexp(1.0, -1060), 0.0), (0.0, np.ldexp(3.0, -1074))],
        "smallest_normal": [(0.0, 0.0), (tiny, 0.0), (0.0, -tiny)],
        "nonfinite": [(np.inf, 1.0), (np.nan, 2.0), (-np.inf, np.nan), (3.0, np.inf)],
        "sum_overflows": [(0.0, 0.0), (1.5e308, 1.5e308), (-1.0e308, 1.7e308)],
    }[kind]
    pos = np.concatenate([base, np.array(extra, F64), base[:3]])  # (and again after them: ascending j around the odd ones)
    vel = rng.uniform(-1, 1, pos.shape)
    w = (np.arange(len(pos)) % 5 + 1).astype(np.uint32)
    return pos, vel, w


@pytest.mark.parametrize("kind", ["coincident", "subnormal", "smallest_normal", "nonfinite", "sum_overflows"])
@pytest.mark.parametrize("arith", ["exact", "auto"])
def test_skip_semantics_bit_for_bit(nb, orc, ctx, kind, arith):
    pos, vel, w = _skip_case(kind)
    _set(ctx, nb._capi, arith)
    ctx.upload(pos, vel, w)
    ref, _ = orc.direct_accel(pos, w, accum="native")
    assert _same_bits(ctx.accel_direct(), ref)
    ctx.update_direct(0.1, 2)
    p, v, _, _ = ctx.download()
    rp, rv, _ = orc.update_direct(pos, vel, w, delta=0.1, nsteps=2)
    assert _same_bits(p, rp) and _same_bits(v, rv)


@pytest.mark.parametrize("kind", ["subnormal", "nonfinite", "sum_overflows"])
def test_fast_outside_its_domain_is_the_exact_step(nb, orc, ctx, kind):
    """Positions outside the FAST domain (non-finite, >= 2^100, non-zero below 2^-300): the step runs EXACT."""
    pos, vel, w = _skip_case(kind)
    _set(ctx, nb._capi, "fast")
    ctx.upload(pos, vel, w)
    ref, _ = orc.direct_accel(pos, w, accum="native")
    assert _same_bits(ctx.accel_direct(), ref)


def test_fast_keeps_1e12_at_65536_and_is_reproducible(nb, orc, ctx):
    n = 65536
    pos, vel, w = _scene(nb, n, 0xD6402)
    _set(ctx, nb._capi, "fast")
    ctx.upload(pos, vel, w)
    acc = ctx.accel_direct()
    ref, norm = orc.direct_accel(pos, w, accum="f64", nthreads=16)
    r = _fast_error(acc, ref, norm)
    print(f"[tol] f64 direct FAST n={n}: median {np.median(r):.2e} max {r.max():.2e}")
    assert np.all(np.isfinite(acc)) and r.max() <= FAST_RTOL, r.max()
    assert not _same_bits(acc, ref)          # (it is the FAST kernel that ran)
    ctx.upload(pos, vel, w)
    assert _same_bits(ctx.accel_direct(), acc)


def test_fast_with_one_nan_position_is_the_exact_step(nb, orc, ctx):
    pos, vel, w = _scene(nb, 4096, 0xD6403)
    pos[1234, 0] = np.nan
    _set(ctx, nb._capi, "fast")
    ctx.upload(pos, vel, w)
    ref, _ = orc.direct_accel(pos, w, accum="native", nthreads=8)
    assert _same_bits(ctx.accel_direct(), ref)
    ctx.update_direct(0.1, 1)
    p, v, _, _ = ctx.download()
    rp, rv, _ = orc.update_direct(pos, vel, w, delta=0.1, nsteps=1, nthreads=8)
    assert _same_bits(p, rp) and _same_bits(v, rv)


def test_fast_trajectory_is_reproducible(nb, ctx):
    pos, vel, w = _scene(nb, 20000, 0xD6404)
    _set(ctx, nb._capi, "fast")
    out = []
    for _ in range(2):
        ctx.upload(pos, vel, w)
        ctx.update_direct(0.1, 3)
        out.append(ctx.download()[:2])
    assert _same_bits(out[0][0], out[1][0]) and _same_bits(out[0][1], out[1][1])


def test_262144_bodies_one_step_sampled_bit_for_bit(nb, orc, ctx):
    n = 262144
    pos, vel, w = _scene(nb, n, 0xD6405)
    _set(ctx, nb._capi, "exact")
    ctx.upload(pos, vel, w)
    acc = ctx.accel_direct()
    idx = np.random.default_rng(3).choice(n, 4096, replace=False)
    ref, _ = orc.direct_accel(pos, w, targets=idx, accum="native", nthreads=16)
    assert _same_bits(acc[idx], ref)
    acc2 = ctx.accel_direct()
    assert _same_bits(acc2, acc)
    ctx.update_direct(0.1, 1)
    p, v, _, _ = ctx.download()
    dt = F64(0.1)
    rv = vel[idx] + ref * dt                 # main.rs:419-423 on the sampled rows, one rounding per operation
    rp = pos[idx] + rv * dt
    assert _same_bits(v[idx], rv) and _same_bits(p[idx], rp)


@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_n_steps_in_one_call_equal_one_call_per_step(nb, orc, ctx, arith):
    pos, vel, w = _scene(nb, 3000, 0xD6406)
    _set(ctx, nb._capi, arith)
    ctx.upload(pos, vel, w)
    ctx.update_direct(0.05, 5)
    a = ctx.download()
    ctx.upload(pos, vel, w)
    for _ in range(5):
        ctx.update_direct(0.05, 1)
    b = ctx.download()
    assert all(_same_bits(x, y) for x, y in zip(a, b))
    if arith == "exact":
        rp, rv, _ = orc.update_direct(pos, vel, w, delta=0.05, nsteps=5, nthreads=8)
        assert _same_bits(a[0], rp) and _same_bits(a[1], rv)


def test_zero_steps_and_zero_bodies_are_no_ops(nb, ctx):
    C = nb._capi
    pos, vel, w = _scene(nb, 100, 0xD6407)
    _set(ctx, C, "exact")
    ctx.upload(pos, vel, w)
    ctx.update_direct(0.1, 0)
    p, v, _, _ = ctx.download()
    assert _same_bits(p, pos) and _same_bits(v, vel)
    ctx.upload(np.zeros((0, 2), F64), np.zeros((0, 2), F64), np.zeros(0, np.uint32))
    ctx.update_direct(0.1, 3)
    assert ctx.accel_direct().shape == (0, 2)


def test_timer_brackets_the_f64_step(nb, ctx):
    C = nb._capi
    pos, vel, w = _scene(nb, 4096, 0xD6408)
    _set(ctx, C, "exact")
    ctx.upload(pos, vel, w)
    t = C.Timer()
    try:
        ctx.set_timer(t)
        ctx.update_direct(0.1, 3)
        ms, launches = t.read()
        assert launches == 3 and ms > 0.0
    finally:
        ctx.set_timer(None)
        t.close()


def test_direct_and_tree_steps_interleave_on_one_context(nb, orc, ctx):
    C = nb._capi
    pos, vel, w = _scene(nb, 2048, 0xD6409)
    w = (np.arange(2048) % 7 + 1).astype(np.uint32)
    _set(ctx, C, "auto", theta=0.5)
    ctx.upload(pos, vel, w)
    ctx.update_direct(0.1, 2)
    ctx.update_tree(C.TREE_BVH, 0.1, 1)
    ctx.update_direct(0.1, 1)
    ctx.update_tree(C.TREE_QUAD, 0.1, 2)
    ctx.update_direct(0.1, 1)
    p, v, w2, ids = ctx.download()
    rp, rv, _ = orc.update_direct(pos, vel, w, delta=0.1, nsteps=2, nthreads=8)
    rp, rv, rw, rids, _ = orc.update_bvh(rp, rv, w, delta=0.1, theta=0.5, mode=orc.AS_WRITTEN, nsteps=1, nthreads=8)
    rp, rv, _ = orc.update_direct(rp, rv, rw, delta=0.1, nsteps=1, nthreads=8)
    rp, rv, _ = orc.update_quad(rp, rv, rw, delta=0.1, theta=0.5, nsteps=2, nthreads=8)
    rp, rv, _ = orc.update_direct(rp, rv, rw, delta=0.1, nsteps=1, nthreads=8)
    assert np.array_equal(ids, rids) and np.array_equal(w2, rw)
    assert _same_bits(p, rp) and _same_bits(v, rv)


def test_world_direct_float64(nb, orc):
    pos, vel, w = _scene(nb, 1500, 0xD640A)
    world = nb.World(pos, vel, w, method="direct", arith="exact")
    try:
        world.update(0.1, None, n_steps=3)
        p, v, _, _ = world.particles()
    finally:
        world.close()
    rp, rv, _ = orc.update_direct(pos, vel, w, delta=0.1, nsteps=3, nthreads=8)
    assert p.dtype == F64 and _same_bits(p, rp) and _same_bits(v, rv)


def test_a_multi_device_context_refuses_f64_direct_steps(nb):
    C = nb._capi
    pos, vel, w = _scene(nb, 1000, 0xD640B)
    m = C.MultiContext([0], C.EXCHANGE_PEER)
    try:
        m.upload(pos, vel, w)
        rc = m.lib.nbody_update_direct_f64(m.h, 0.1, 1, None)
        assert rc == C.ERR_INVALID and b"multi-device direct steps are f32 only" in m.lib.nbody_last_error(m.h)
        with pytest.raises(C.NBodyError, match="multi-device direct steps are f32 only"):
            m.accel_direct()
    finally:
        m.close()
