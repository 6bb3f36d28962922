"""The direct sum at arbitrary points (nbody_accel_direct_at_f32 / _f64, Context.accel_direct(targets)) against the CPU oracle's
direct_accel(..., target_pos=P).

EXACT is bit-identical to one ascending-row chain per target, in f32 and f64, skip cases and all; FAST is within the step's
contract (f32: tests/_tol.py ACC_RTOL, f64: 1e-12 of sum_j |term_ij|_1); AUTO routes as the header says; and a target's bits
depend on its own position alone — not on the other targets, their order or number, nor on the devices of a multi-device
context.  Needs an MI355X."""
import numpy as np
import pytest

from _tol import check_fast

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
FAST64_RTOL = 1e-12
NTH = 16


@pytest.fixture(scope="module")
def ctx(nb):
    c = nb._capi.Context(0)
    yield c
    c.close()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.uint64 if a.dtype == F64 else np.uint32
    return np.array_equal(a.view(u), b.view(u))


def _set(ctx, C, arith, **kw):
    ctx.set_params(arith={"auto": C.ARITH_AUTO, "fast": C.ARITH_FAST, "exact": C.ARITH_EXACT}[arith], **kw)


def _skip_cases(dt):
    tiny = np.finfo(dt).tiny
    big = 3e38 if dt == F32 else 1.5e308
    sub = 1e-39 if dt == F32 else 1e-310
    return np.array([[0, 0], [-0.0, 0.0], [sub, 0], [0, -sub], [tiny, 0], [np.inf, 1], [-np.inf, 0], [np.nan, 2],
                     [big, big], [-big, -big], [2.0 ** 60, 5], [2.0 ** 61, -(2.0 ** 62)], [3, 4], [0.01, 0.0]], dt)


def _targets(rng, pos, clamp, dt, n_random=1024, n_on=64, n_near=64):
    """Random points over the bodies' box, points exactly on bodies, points at 0.5 sqrt(clamp) from bodies, the skip cases."""
    fin = pos[np.all(np.isfinite(pos), axis=1)].astype(F64)
    lo, hi = fin.min(axis=0), fin.max(axis=0)
    rnd = lo + (hi - lo) * rng.random((n_random, 2))
    on = pos[rng.integers(0, len(pos), n_on)].astype(F64)
    ang = rng.random(n_near) * 2 * np.pi
    near = pos[rng.integers(0, len(pos), n_near)].astype(F64) + 0.5 * np.sqrt(clamp) * np.stack([np.cos(ang), np.sin(ang)], 1)
    return np.concatenate([rnd, on, near]).astype(dt), _skip_cases(dt)


def _exact_ref(orc, pos, w, tgt, clamp=0.001):
    ref, _ = orc.direct_accel(pos, w, target_pos=tgt, clamp=clamp, accum="native", nthreads=NTH)
    return ref.astype(pos.dtype)


def _scene(nb, n, dt, seed):
    pos, vel, w = nb.scenes.plummer(n, seed=seed, dtype=dt)
    return pos, vel, w


# ---- 1. EXACT bit parity
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("n", [1, 63, 1024, 65537, "galaxy"])
def test_exact_is_the_oracles_sum_bit_for_bit(nb, orc, ctx, dt, n):
    C = nb._capi
    if n == "galaxy":
        pos, vel, w = nb.scenes.galaxy(dtype=dt)
        pos, vel, w = pos.astype(dt), vel.astype(dt), w
    else:
        pos, vel, w = _scene(nb, n, dt, 0xA7 + (n if isinstance(n, int) else 0))
        if n >= 1024:
            w = np.random.default_rng(n).integers(1, 1000, len(w)).astype(np.uint32)
    _set(ctx, C, "exact")
    ctx.upload(pos, vel, w)
    rng = np.random.default_rng(17)
    tgt, skip = _targets(rng, pos, 0.001, dt, n_random=512 if len(pos) > 10000 else 1024)
    if n == "galaxy":  # the two heavy bodies: on them and next to them
        heavy = pos[:2].astype(F64)
        tgt = np.concatenate([tgt, heavy.astype(dt), (heavy + 0.5 * np.sqrt(0.001)).astype(dt), (heavy + 100.0).astype(dt)])
    for t in (tgt, skip):
        acc = ctx.accel_direct(t)
        assert acc.dtype == dt and acc.shape == t.shape
        assert _same(acc, _exact_ref(orc, pos, w, t))


@pytest.mark.parametrize("dt", [F32, F64])
def test_exact_with_skip_case_bodies(nb, orc, ctx, dt):
    """Bodies at the skip cases too (NaN, inf, subnormal, overflowing sums), targets everywhere: still bit for bit."""
    C = nb._capi
    pos = _skip_cases(dt)
    w = np.arange(1, len(pos) + 1, dtype=np.uint32) * 3
    for arith in ("exact", "auto"):
        _set(ctx, C, arith)
        ctx.upload(pos, np.zeros_like(pos), w)
        tgt = np.concatenate([pos, np.array([[1, 1], [-2.5, 7], [1e-30, 0]], dt)])
        assert _same(ctx.accel_direct(tgt), _exact_ref(orc, pos, w, tgt)), arith


# ---- 2. the bodies' own positions
@pytest.mark.parametrize("dt", [F32, F64])
def test_targets_at_the_bodies_equal_accel_direct(nb, ctx, dt):
    C = nb._capi
    pos, vel, _ = _scene(nb, 4096, dt, 0xB0D)
    w = np.random.default_rng(5).integers(1, 50, 4096).astype(np.uint32)
    _set(ctx, C, "exact")
    ctx.upload(pos, vel, w)
    assert _same(ctx.accel_direct(pos), ctx.accel_direct())


# ---- 3. FAST within the contract
def _check_fast32(orc, pos, w, tgt, acc, clamp=0.001):
    ref64, norm = orc.direct_accel(pos, w, target_pos=tgt, clamp=clamp, accum="f64", nthreads=NTH)
    check_fast(acc, ref64, norm)


@pytest.mark.parametrize("case", ["plummer", "free_masses", "reference_scene"])
def test_fast_f32_within_tolerance(nb, orc, ctx, case):
    C = nb._capi
    rng = np.random.default_rng(23)
    if case == "reference_scene":
        pos, vel, w = nb.scenes.galaxy()
        tgt, _ = _targets(rng, pos, 0.001, F32, n_random=8192)
        heavy = pos[:2].astype(F64)
        tgt = np.concatenate([tgt, (heavy + 0.5 * np.sqrt(0.001)).astype(F32), (heavy + 3.0).astype(F32)])
    else:
        pos, vel, w = _scene(nb, 65536, F32, 0xFA57)
        if case == "free_masses":
            w = rng.integers(1, 100000, 65536).astype(np.uint32)
        tgt = np.concatenate([pos, _targets(rng, pos, 0.001, F32, n_random=0)[0]])
    ref64, norm = orc.direct_accel(pos, w, target_pos=tgt, accum="f64", nthreads=NTH)
    for arith in ("fast", "auto"):
        _set(ctx, C, arith)
        ctx.upload(pos, vel, w)
        acc = ctx.accel_direct(tgt)
        check_fast(acc, ref64, norm)
    assert not _same(acc[:512], _exact_ref(orc, pos, w, tgt[:512]))  # FAST really ran


def test_fast_f32_2pow20_targets_over_2pow20_bodies(nb, orc, ctx):
    C = nb._capi
    pos, vel, w = _scene(nb, 1 << 20, F32, 0x1F1F)
    rng = np.random.default_rng(29)
    tgt = (pos + rng.normal(0, 1, pos.shape)).astype(F32)
    _set(ctx, C, "auto")
    ctx.upload(pos, vel, w)
    acc = ctx.accel_direct(tgt)
    assert np.all(np.isfinite(acc))
    pick = rng.choice(len(tgt), 1024, replace=False)
    _check_fast32(orc, pos, w, tgt[pick], acc[pick])


def test_fast_f64_within_1e_12(nb, orc, ctx):
    C = nb._capi
    pos, vel, _ = _scene(nb, 65536, F64, 0xF64)
    w = np.random.default_rng(31).integers(1, 1000, 65536).astype(np.uint32)
    rng = np.random.default_rng(37)
    tgt = (pos + rng.normal(0, 2, pos.shape)).astype(F64)
    tgt[:128] = pos[1000:1128]  # some on bodies
    _set(ctx, C, "fast")
    ctx.upload(pos, vel, w)
    acc = ctx.accel_direct(tgt)
    ref, norm = orc.direct_accel(pos, w, target_pos=tgt, accum="f64", nthreads=NTH)
    err = np.abs(acc - ref).sum(axis=1) / np.maximum(norm, 1e-300)
    assert np.all(np.isfinite(err)) and err.max() <= FAST64_RTOL, err.max()
    assert not _same(acc[:512], _exact_ref(orc, pos, w, tgt[:512]))


# ---- 4. per-target determinism
@pytest.mark.parametrize("dt", [F32, F64])
@pytest.mark.parametrize("arith", ["fast", "exact"])
def test_a_target_depends_on_its_position_alone(nb, ctx, dt, arith):
    C = nb._capi
    pos, vel, _ = _scene(nb, 65536, dt, 0xDE7)
    w = np.random.default_rng(41).integers(1, 1000, 65536).astype(np.uint32)
    _set(ctx, C, arith)
    ctx.upload(pos, vel, w)
    rng = np.random.default_rng(43)
    tgt = np.concatenate([_targets(rng, pos, 0.001, dt, n_random=3000)[0], pos[:500]])
    ref = ctx.accel_direct(tgt)
    perm = rng.permutation(len(tgt))
    assert _same(ctx.accel_direct(tgt[perm]), ref[perm])
    h = len(tgt) // 2
    assert _same(np.concatenate([ctx.accel_direct(tgt[:h]), ctx.accel_direct(tgt[h:])]), ref)
    for i in rng.choice(len(tgt), 16, replace=False):
        assert _same(ctx.accel_direct(tgt[i:i + 1]), ref[i:i + 1]), i
    # 2^20 + 37 others first: a call of several batches, and the set off every batch, block and wave boundary it had alone
    other = (rng.random(((1 << 20) + 37, 2)) * 1e5).astype(dt)
    big = ctx.accel_direct(np.concatenate([other, tgt]))
    assert _same(big[len(other):], ref)


# ---- 5. AUTO routing
def test_auto_f32_hazardous_targets_take_their_exact_values(nb, orc, ctx):
    C = nb._capi
    pos, vel, w = _scene(nb, 65536, F32, 0xA070)
    rng = np.random.default_rng(47)
    fin = _targets(rng, pos, 0.001, F32, n_random=2000)[0]
    bad = np.array([[np.nan, 1.0], [2.0 ** 61, 3.0]], F32)
    _set(ctx, C, "auto")
    ctx.upload(pos, vel, w)
    plain = ctx.accel_direct(fin)
    mixed = ctx.accel_direct(np.concatenate([fin[:700], bad[:1], fin[700:1500], bad[1:], fin[1500:]]))
    assert _same(np.concatenate([mixed[:700], mixed[701:1501], mixed[1502:]]), plain)
    ex = _exact_ref(orc, pos, w, bad)
    assert _same(mixed[[700, 1501]], ex)
    assert not _same(plain, _exact_ref(orc, pos, w, fin))  # the finite ones ran FAST
    _set(ctx, C, "exact")
    assert _same(ctx.accel_direct(bad), ex)


def test_auto_f32_a_nan_body_makes_every_target_exact(nb, orc, ctx):
    C = nb._capi
    pos, vel, w = _scene(nb, 65536, F32, 0xA071)
    pos[1234] = (np.nan, 5.0)
    tgt = _targets(np.random.default_rng(53), pos, 0.001, F32, n_random=1000)[0]
    _set(ctx, C, "auto")
    ctx.upload(pos, vel, w)
    assert _same(ctx.accel_direct(tgt), _exact_ref(orc, pos, w, tgt))


def test_f64_auto_is_exact_and_fast_routes_like_the_step(nb, orc, ctx):
    C = nb._capi
    pos, vel, w = _scene(nb, 8192, F64, 0xA072)
    tgt = _targets(np.random.default_rng(59), pos, 0.001, F64, n_random=1000)[0]
    _set(ctx, C, "auto")
    ctx.upload(pos, vel, w)
    assert _same(ctx.accel_direct(tgt), _exact_ref(orc, pos, w, tgt))
    _set(ctx, C, "fast")
    bad = np.array([[np.nan, 1.0], [2.0 ** 101, 0.0], [1e-305, 1.0]])
    plain = ctx.accel_direct(tgt)
    mixed = ctx.accel_direct(np.concatenate([tgt, bad]))
    assert _same(mixed[:len(tgt)], plain) and _same(mixed[len(tgt):], _exact_ref(orc, pos, w, bad))
    p2 = pos.copy()
    p2[77] = (np.inf, 0.0)
    ctx.upload(p2, vel, w)
    assert _same(ctx.accel_direct(tgt), _exact_ref(orc, p2, w, tgt))


# ---- 6. after BVH steps (rows permuted)
@pytest.mark.parametrize("dt", [F32, F64])
def test_after_bvh_steps_parity_on_the_downloaded_rows(nb, orc, ctx, dt):
    C = nb._capi
    pos, vel, _ = _scene(nb, 8192, dt, 0xB7)
    w = np.random.default_rng(61).integers(1, 1000, 8192).astype(np.uint32)
    _set(ctx, C, "exact", theta=0.5, order=C.ORDER_AS_WRITTEN)
    ctx.upload(pos, vel, w)
    ctx.update_tree(C.TREE_BVH, 0.1, 5)
    p, _, w2, ids = ctx.download()
    assert not np.array_equal(ids, np.arange(8192))
    tgt = _targets(np.random.default_rng(67), p, 0.001, dt, n_random=1000)[0]
    assert _same(ctx.accel_direct(tgt), _exact_ref(orc, p, w2, tgt))


# ---- 7. state untouched
@pytest.mark.parametrize("arith", ["auto", "exact"])
def test_the_call_leaves_the_state_alone(nb, ctx, arith):
    C = nb._capi
    pos, vel, w = _scene(nb, 4096, F32, 0x57A7)
    tgt = _targets(np.random.default_rng(71), pos, 0.001, F32, n_random=5000)[0]
    runs = []
    for probe in (False, True):
        _set(ctx, C, arith)
        ctx.upload(pos, vel, w)
        ctx.update_direct(0.1, 4)  # (the captured step pair)
        before = ctx.download()
        cnt0 = ctx.counting()
        if probe:
            ctx.accel_direct(tgt)
            cnt1 = ctx.counting()
            assert (cnt1.build_bvh, cnt1.sum_gravity, cnt1.post_calculations) == \
                   (cnt0.build_bvh, cnt0.sum_gravity, cnt0.post_calculations)
            for a, b in zip(ctx.download(), before):
                assert _same(a, b)
        ctx.update_direct(0.1, 5)
        runs.append((before, ctx.download()))
    for (b0, a0), (b1, a1) in zip([runs[0]], [runs[1]]):
        for x, y in zip(b0 + a0, b1 + a1):
            assert _same(x, y)


# ---- 8. multi-device rehearsal on one GPU
@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("dt", [F32, F64])
def test_multi_device_context_equals_a_single_context(nb, ctx, ranks, dt):
    C = nb._capi
    pos, vel, _ = _scene(nb, 20000, dt, 0x3D)
    w = np.random.default_rng(73).integers(1, 1000, 20000).astype(np.uint32)
    tgt = _targets(np.random.default_rng(79), pos, 0.001, dt, n_random=7001)[0]
    m = C.MultiContext([0] * ranks, C.EXCHANGE_PEER)
    try:
        for arith in ("fast", "auto"):
            _set(m, C, arith, theta=0.5)
            _set(ctx, C, arith, theta=0.5)
            m.upload(pos, vel, w)
            for stage in ("upload", "step"):
                if stage == "step":
                    if dt == F32:
                        m.update_direct(0.1, 1)
                    else:
                        m.update_tree(C.TREE_BVH, 0.1, 1)
                p, v, w2, _ = m.download()
                ctx.upload(p, v, w2)
                assert _same(m.accel_direct(tgt), ctx.accel_direct(tgt)), (arith, stage)
    finally:
        m.close()


# ---- 9. errors
def test_invalid_calls_and_empty_cases(nb, ctx):
    C = nb._capi
    lib = ctx.lib
    t32, a32 = np.ones((2, 2), F32), np.zeros((2, 2), F32)
    t64, a64 = np.ones((2, 2), F64), np.zeros((2, 2), F64)

    def call(f, h, n, t, a):
        return f(h, n, None if t is None else C._ptr(t), None if a is None else C._ptr(a))

    fresh = C.Context(0)
    try:
        assert call(lib.nbody_accel_direct_at_f32, fresh.h, 2, t32, a32) == C.ERR_INVALID
        assert b"no particles" in lib.nbody_last_error(fresh.h)
        assert call(lib.nbody_accel_direct_at_f64, fresh.h, 2, t64, a64) == C.ERR_INVALID
    finally:
        fresh.close()
    pos, vel, w = _scene(nb, 256, F32, 0xE)
    _set(ctx, C, "auto")
    ctx.upload(pos, vel, w)
    f32, f64 = lib.nbody_accel_direct_at_f32, lib.nbody_accel_direct_at_f64
    assert call(f32, ctx.h, -1, t32, a32) == C.ERR_INVALID and b"n_targets < 0" in lib.nbody_last_error(ctx.h)
    assert call(f32, ctx.h, 2, None, a32) == C.ERR_INVALID and b"NULL" in lib.nbody_last_error(ctx.h)
    assert call(f32, ctx.h, 2, t32, None) == C.ERR_INVALID and b"NULL" in lib.nbody_last_error(ctx.h)
    assert call(f64, ctx.h, 2, t64, a64) == C.ERR_INVALID and b"other precision" in lib.nbody_last_error(ctx.h)
    assert call(f32, ctx.h, 0, None, None) == C.OK
    assert ctx.accel_direct(np.zeros((0, 2), F32)).shape == (0, 2)
    ctx.upload(pos.astype(F64), vel.astype(F64), w)
    assert call(f32, ctx.h, 2, t32, a32) == C.ERR_INVALID and b"other precision" in lib.nbody_last_error(ctx.h)
    assert call(f64, ctx.h, 0, None, None) == C.OK
    for dt in (F32, F64):  # zero bodies: +0 everywhere
        ctx.upload(np.zeros((0, 2), dt), np.zeros((0, 2), dt), np.zeros(0, np.uint32))
        acc = ctx.accel_direct(np.array([[1, 2], [np.nan, 0]], dt))
        assert _same(acc, np.zeros((2, 2), dt))
