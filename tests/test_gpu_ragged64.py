"""Ragged ensembles in f64 on the device (nb.RaggedEnsemble64 over nbody_ragged64_*): double-precision worlds of different sizes
stepped together.  Every world is compared on its own — EXACT and AUTO with the oracle's update_direct of that world alone on
float64, bit for bit; FAST with nb.Ensemble64 holding that world alone, bit for bit (the two kernels share one body), and with
the contract of DESIGN §5, |a - a_ref|_1 <= 1e-12 * sum_j |term_ij|_1 per body.  Needs an MI355X.

Sizes: odd ones early, so that later worlds start at odd rows; sizes that are no multiple of the term block of 8; 128 / 129 and
256 / 257 on either side of a lane split and of a launch class; one size inside every range of ensemble_split; 3272 / 3273 on
either side of the 64 KiB dynamic-LDS limit (65 440 / 65 600 B), which the ragged kernel has to have raised for itself; 4096,
the top size (16 blocks, 81 920 B of LDS).  In every FAST world body 0 has a weight >= 2: its LDS word is the one borrowed for
the route, and a weight that came back as the route's 0 or 1 would show."""
import numpy as np
import pytest

from tests.test_gpu_ensemble64 import (FAST_RTOL, _awkward_world, _fast_error, _fast_worlds, _outside_domain, _routed_worlds,
                                       _same_bits, _uneven_weights)

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64

MIXED = [300, 1, 65, 4096, 2, 257, 63, 128, 129, 1000, 7, 64, 256, 12, 3]
EVERY_SIZE = [1, 3, 7, 129, 257, 2, 12, 24, 50, 100, 128, 256, 300, 1000, 3273, 3272, 4096]


def _worlds(nb, sizes, seed, awkward_at=()):
    """One float64 world per size from distinct seeds (Plummer sets with uneven weights); the worlds at `awkward_at` are the f64
    ensemble test's _awkward_world.  Body 0 of every world weighs at least 2."""
    ps, vs, ws = [], [], []
    for k, n in enumerate(sizes):
        if k in awkward_at:
            p, v, w = _awkward_world(n)
        else:
            p, v, _ = nb.scenes.plummer(n, seed=seed + k, dtype=F64)
            w = _uneven_weights(n, seed + k)
        w[0] = max(int(w[0]), 2)
        assert p.dtype == F64 and v.dtype == F64 and w.dtype == np.uint32
        ps.append(np.ascontiguousarray(p)), vs.append(np.ascontiguousarray(v)), ws.append(w)
    return ps, vs, ws


def _oracle_steps(orc, pos, vel, w, steps, clamp=0.001, delta=0.1):
    out = [orc.update_direct(pos[k], vel[k], w[k], delta=delta, clamp=clamp, nsteps=steps, nthreads=16)[:2] for k in range(len(pos))]
    assert out[0][0].dtype == F64
    return [o[0] for o in out], [o[1] for o in out]


def _assert_worlds_equal(got, want, what):
    assert len(got) == len(want), what
    for k in range(len(want)):
        assert _same_bits(got[k], want[k]), f"{what}: world {k} (n = {len(want[k])}) differs"


def _ragged_run(nb, pos, vel, w, arith, steps, clamp=0.001):
    with nb.RaggedEnsemble64(pos, vel, w, arith=arith, clamp=clamp) as ens:
        ens.update(0.1, None, n_steps=steps)
        p, v, _ = ens.particles()
        return p, v, ens.accel()


def _uniform_run(nb, p, v, w, arith, steps, clamp=0.001):
    """nb.Ensemble64 holding this one world -> its positions, velocities after `steps` steps and the accelerations there."""
    with nb.Ensemble64(p[None], v[None], w[None], arith=arith, clamp=clamp) as ens:
        ens.update(0.1, None, n_steps=steps)
        pp, vv, _ = ens.particles()
        return pp[0], vv[0], ens.accel()[0]


# ------------------------------------------------------------------ 1. EXACT and AUTO, mixed sizes
@pytest.fixture(scope="module")
def mixed(nb, orc):
    """The mixed worlds and their oracle, computed once: 3 steps of every world alone and the accelerations after them."""
    pos, vel, w = _worlds(nb, MIXED, seed=2100, awkward_at=(5,))
    rp, rv = _oracle_steps(orc, pos, vel, w, 3)
    ra = [orc.direct_accel(rp[k], w[k], accum="native", nthreads=16)[0] for k in range(len(MIXED))]
    return pos, vel, w, rp, rv, ra


@pytest.mark.parametrize("arith", ["exact", "auto"])
def test_exact_and_auto_mixed_sizes_every_world_bit_identical_to_its_oracle(nb, mixed, arith):
    pos, vel, w, rp, rv, ra = mixed
    with nb.RaggedEnsemble64(pos, vel, w, arith=arith) as ens:
        assert ens.sizes == MIXED and ens.h.shape == (len(MIXED), sum(MIXED)) and ens.h.sizes.tolist() == MIXED
        ens.update(0.1, None, n_steps=3)
        p, v, w2 = ens.particles()
        assert [a.shape for a in p] == [(n, 2) for n in MIXED] and [a.shape for a in w2] == [(n,) for n in MIXED]
        assert all(a.dtype == F64 for a in p + v)
        _assert_worlds_equal(p, rp, "positions")
        _assert_worlds_equal(v, rv, "velocities")
        assert all(np.array_equal(a, b) for a, b in zip(w2, w))
        acc = ens.accel()
        for k in range(len(MIXED)):
            assert acc[k].dtype == F64 and _same_bits(acc[k], ra[k]), k
        p2, v2, _ = ens.particles()                       # accel() left the state's bits alone
        assert all(a.tobytes() == b.tobytes() for a, b in zip(p2 + v2, p + v))
    assert not np.array_equal(p[0], pos[0])               # (and something moved)


def test_default_arith_is_the_exact_chain(nb, mixed):
    pos, vel, w, rp, rv, _ = mixed
    keep = [0, 1, 2, 4, 5]
    with nb.RaggedEnsemble64([pos[k] for k in keep], [vel[k] for k in keep], [w[k] for k in keep]) as ens:
        assert ens.h.get_params().arith == nb._capi.ARITH_EXACT
        ens.update(0.1, None, n_steps=3)
        p, v, _ = ens.particles()
    _assert_worlds_equal(p, [rp[k] for k in keep], "positions")
    _assert_worlds_equal(v, [rv[k] for k in keep], "velocities")


# ------------------------------------------------------------------ 2. FAST equals the uniform f64 ensemble, bit for bit
def test_fast_every_world_bit_identical_to_the_uniform_ensemble(nb):
    sizes = list(EVERY_SIZE)
    pos, vel, w = _worlds(nb, sizes, seed=2200)
    assert all(int(ww[0]) >= 2 for ww in w)
    p, v, acc = _ragged_run(nb, pos, vel, w, "fast", 3)
    for k, n in enumerate(sizes):
        up, uv, ua = _uniform_run(nb, pos[k], vel[k], w[k], "fast", 3)
        assert _same_bits(p[k], up) and _same_bits(v[k], uv), f"n = {n}: state differs from nb.Ensemble64 of that world alone"
        assert _same_bits(acc[k], ua), f"n = {n}: accel differs from nb.Ensemble64 of that world alone"
        assert n == 1 or not np.array_equal(p[k], pos[k]), n


# ------------------------------------------------------------------ 3. FAST within the frozen 1e-12
@pytest.fixture(scope="module")
def galaxy64(nb):
    return nb.scenes.galaxy(dtype=F64)


def test_fast_accel_within_1e12(nb, orc, galaxy64):
    per_n = [_fast_worlds(nb, galaxy64, n) for n in (64, 1000, 4096)]      # each (pos[3,n,2], vel[3,n,2], w[3,n])
    pos, vel, w = ([np.ascontiguousarray(per_n[i][x][j]) for j in range(3) for i in range(3)] for x in range(3))
    sizes = [len(p) for p in pos]
    assert sizes == [64, 1000, 4096] * 3                                   # interleaved: 64, 1000, 4096, 64, 1000, ...
    for ww in w:
        ww[0] = max(int(ww[0]), 2)                                         # (the close-pairs world has a body 0 of weight 1)
    with nb.RaggedEnsemble64(pos, vel, w, arith="fast") as ens:
        acc = ens.accel()
        again = ens.accel()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(acc, again))
    assert FAST_RTOL == 1e-12
    for k, n in enumerate(sizes):
        ref, norm = orc.direct_accel(pos[k], w[k], accum="f64", nthreads=16)
        assert np.all(np.isfinite(acc[k])), k
        r = _fast_error(acc[k], ref, norm)
        print(f"[tol] f64 ragged FAST n={n} world {k}: max {r:.2e}")
        assert r <= FAST_RTOL, (n, k, r)                                   # no body left out
        if n > 64:
            native, _ = orc.direct_accel(pos[k], w[k], accum="native", nthreads=16)
            assert not _same_bits(acc[k], native), (n, k)                  # i.e. FAST really ran


# ------------------------------------------------------------------ 4. equal sizes through the ragged route
@pytest.mark.parametrize("arith", ["fast", "exact"])
def test_equal_sizes_through_the_ragged_kernel_equal_the_uniform_ensemble(nb, arith):
    pos, vel, w = _worlds(nb, [300] * 5, seed=2300, awkward_at=(1,))
    p, v, acc = _ragged_run(nb, pos, vel, w, arith, 5)
    with nb.Ensemble64(np.stack(pos), np.stack(vel), np.stack(w), arith=arith) as ens:
        ens.update(0.1, None, n_steps=5)
        up, uv, _ = ens.particles()
        ua = ens.accel()
    _assert_worlds_equal(p, list(up), "positions")
    _assert_worlds_equal(v, list(uv), "velocities")
    _assert_worlds_equal(acc, list(ua), "accel")
    assert not np.array_equal(p[0], pos[0])


# ------------------------------------------------------------------ 5. independence
@pytest.mark.parametrize("arith", ["fast", "exact"])
def test_a_world_depends_on_nothing_but_itself(nb, arith):
    sizes = [300, 7, 129, 300, 64, 1000, 2, 128]
    pos, vel, w = _worlds(nb, sizes, seed=2400, awkward_at=(3,))   # (under FAST world 3 routes to EXACT, its neighbours do not)
    b = len(sizes)
    p0, v0, _ = _ragged_run(nb, pos, vel, w, arith, 3)
    # reversed
    pr, vr, _ = _ragged_run(nb, pos[::-1], vel[::-1], w[::-1], arith, 3)
    for k in range(b):
        assert _same_bits(p0[k], pr[b - 1 - k]) and _same_bits(v0[k], vr[b - 1 - k]), k
    # a subset: other launches are empty now, and every row0 has changed
    keep = [1, 3, 5, 6]
    ps, vs, _ = _ragged_run(nb, [pos[k] for k in keep], [vel[k] for k in keep], [w[k] for k in keep], arith, 3)
    for i, k in enumerate(keep):
        assert _same_bits(p0[k], ps[i]) and _same_bits(v0[k], vs[i]), k
    # neighbours of another size: world 2 grows from 129 to 4096 (another launch class, 16 blocks where there was one, and the
    # launch that needs the raised LDS limit), world 4 from 64 to 65 (another lane split, and with it another LDS for the launch
    # it shares with worlds 1, 6 and 7); every row after them shifts
    pos2, vel2, w2 = list(pos), list(vel), list(w)
    for k, n in ((2, 4096), (4, 65)):
        pk, vk, wk = _worlds(nb, [n], seed=2460 + k)
        pos2[k], vel2[k], w2[k] = pk[0], vk[0], wk[0]
    pn, vn, _ = _ragged_run(nb, pos2, vel2, w2, arith, 3)
    for k in range(b):
        if k not in (2, 4):
            assert _same_bits(p0[k], pn[k]) and _same_bits(v0[k], vn[k]), k
        assert not np.array_equal(p0[k], pos[k])


# ------------------------------------------------------------------ 6. FAST routes per world
@pytest.mark.parametrize("poison", [1e-305, np.inf, 2.0 ** 100])
def test_fast_routes_each_world_on_its_own(nb, orc, poison):
    # worlds 0, 1, 2 are the f64 ensemble test's three worlds of 200, world 1 poisoned; 3 .. 6 are added: 256 and 130 share its
    # launch class (129 .. 256), 1000 and 50 do not
    rp3, rv3, rw3 = _routed_worlds(nb, poison)
    xp, xv, xw = _worlds(nb, [256, 1000, 50, 130], seed=2500)
    pos, vel, w = [a for a in rp3] + xp, [a for a in rv3] + xv, [a for a in rw3] + xw
    assert all(int(ww[0]) >= 2 for ww in w)
    b = len(pos)
    assert _outside_domain(pos[1][7, 0])
    rp1, _ = _oracle_steps(orc, pos, vel, w, 1)
    rp, rv = _oracle_steps(orc, pos, vel, w, 2)
    assert _outside_domain(rp1[1][7, 0]) and _outside_domain(rp[1][7, 0])   # still outside at the second step and at accel()
    for k in range(b):
        if k != 1:
            assert not any(_outside_domain(x) for x in rp1[k].ravel()) and not any(_outside_domain(x) for x in rp[k].ravel()), k
    pa, va, acc = _ragged_run(nb, pos, vel, w, "fast", 2)
    assert _same_bits(pa[1], rp[1]) and _same_bits(va[1], rv[1])
    for k in range(b):
        if k != 1:
            up, uv, _ = _uniform_run(nb, pos[k], vel[k], w[k], "fast", 2)
            assert _same_bits(pa[k], up) and _same_bits(va[k], uv), k
    # the routes themselves, in the accelerations of the third step: world 1 EXACT, the others not
    for k in range(b):
        ref, _ = orc.direct_accel(pa[k], w[k], accum="native", nthreads=16)
        assert _same_bits(acc[k], ref) == (k == 1), k
    # a clamp that is not > 0: every world EXACT
    rp, rv = _oracle_steps(orc, pos, vel, w, 2, clamp=0.0)
    pa, va, _ = _ragged_run(nb, pos, vel, w, "fast", 2, clamp=0.0)
    _assert_worlds_equal(pa, rp, "clamp 0 positions")
    _assert_worlds_equal(va, rv, "clamp 0 velocities")


# ------------------------------------------------------------------ 7. the launch above 64 KiB of dynamic LDS
def test_the_large_lds_launch(nb, orc):
    """One launch of 81 920 B (its largest member is 4096) that also holds 3272, the last size under 64 KiB, and 3273, the first
    above it.  The ragged handle goes first: no nb.Ensemble64 exists in this test before the ragged steps are done, and the
    uniform kernel's raised limit would not cover the ragged kernel anyway — it is another function."""
    sizes = [3273, 2049, 4096, 3272]
    pos, vel, w = _worlds(nb, sizes, seed=2700)
    assert nb.ragged_plan(sizes, dtype=F64)["lds_bytes"].tolist() == [81920]
    with nb.RaggedEnsemble64(pos, vel, w, arith="exact") as ens:
        ens.update(0.1, None, n_steps=1)
        pe, ve, _ = ens.particles()
        ens.upload(pos, vel, w)
        ens.h.set_params(arith=nb._capi.ARITH_FAST)
        ens.update(0.1, None, n_steps=1)
        pf, vf, _ = ens.particles()
        af = ens.accel()
    rp, rv = _oracle_steps(orc, pos, vel, w, 1)
    _assert_worlds_equal(pe, rp, "EXACT positions")
    _assert_worlds_equal(ve, rv, "EXACT velocities")
    for k, n in enumerate(sizes):
        up, uv, ua = _uniform_run(nb, pos[k], vel[k], w[k], "fast", 1)
        assert _same_bits(pf[k], up) and _same_bits(vf[k], uv) and _same_bits(af[k], ua), n
        assert not _same_bits(pf[k], pe[k]), n                              # FAST really ran


# ------------------------------------------------------------------ 8. buffers and call order
@pytest.mark.parametrize("arith", ["fast", "exact"])
def test_steps_split_over_calls_and_a_second_upload(nb, orc, arith):
    sizes = [257, 3, 129, 64]
    pos, vel, w = _worlds(nb, sizes, seed=2600)

    def state(ens):
        p, v, _ = ens.particles()
        return b"".join(a.tobytes() for a in p + v)

    with nb.RaggedEnsemble64(pos, vel, w, arith=arith) as ens:
        ens.update(0.1, None, n_steps=5)                         # an odd count: ends on the other buffer
        s5 = state(ens)
        ens.upload(pos, vel, w)
        for _ in range(5):
            ens.update(0.1, None, n_steps=1)
        s1 = state(ens)
        ens.upload(pos, vel, w)
        ens.update(0.1, None, n_steps=2)
        s2 = state(ens)
        ens.update(0.1, None, n_steps=0)
        assert state(ens) == s2
        ens.update(0.1, None, n_steps=3)
        s23 = state(ens)
        assert s5 == s1 == s23 and s2 != s5
        if arith == "exact":
            rp, rv = _oracle_steps(orc, pos, vel, w, 5)
            p, v, _ = ens.particles()
            _assert_worlds_equal(p, rp, "5 steps")
            _assert_worlds_equal(v, rv, "5 steps")
        # other sizes on the same handle: more worlds, more rows, other launches
        sizes2 = [65, 1025, 2, 300, 65]
        pos, vel, w = _worlds(nb, sizes2, seed=2650, awkward_at=(0,))
        ens.upload(pos, vel, w)
        assert ens.sizes == sizes2 and ens.h.shape == (5, sum(sizes2))
        ens.h.set_params(arith=nb._capi.ARITH_EXACT)
        ens.update(0.1, None, n_steps=3)
        p, v, w2 = ens.particles()
        rp, rv = _oracle_steps(orc, pos, vel, w, 3)
        _assert_worlds_equal(p, rp, "second upload")
        _assert_worlds_equal(v, rv, "second upload")
        assert all(np.array_equal(a, b) for a, b in zip(w2, w))


def test_call_order_and_booking(nb, orc):
    C = nb._capi
    h = C.Ragged64Handle(0)
    try:
        assert h.shape == (0, 0) and h.sizes.tolist() == []
        for call in (lambda: h.update(0.1, 1), lambda: h.update(0.1, 0), h.accel, h.download):
            with pytest.raises(C.NBodyError) as e:
                call()
            assert e.value.code == C.ERR_INVALID and "ragged" in str(e.value)
        for bad in ([4, 4097], [0, 4], []):
            n = max(sum(bad), 1)
            with pytest.raises(C.NBodyError) as e:
                h.upload(np.array(bad, np.int64), np.zeros((n, 2), F64), np.zeros((n, 2), F64), None)
            assert e.value.code == C.ERR_INVALID and "ragged" in str(e.value) and h.shape == (0, 0)
    finally:
        h.close()

    sizes = [200, 9, 600]
    pos, vel, w = _worlds(nb, sizes, seed=2800)
    cnt = nb.Counting()
    with nb.RaggedEnsemble64(pos, vel, None, arith="auto") as ens:    # no weights: all 1
        ens.update(0.1, cnt, n_steps=0)
        p, v, w1 = ens.particles()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(p + v, pos + vel)) and cnt.sum_gravity == 0.0
        assert all(a.dtype == np.uint32 and (a == 1).all() for a in w1)
        with pytest.raises(C.NBodyError) as e:
            ens.update(0.1, None, n_steps=-1)
        assert e.value.code == C.ERR_INVALID and "ragged" in str(e.value)
        ens.update(0.1, cnt, n_steps=2)
        assert cnt.sum_gravity > 0.0 and cnt.build_bvh == 0.0 and cnt.post_calculations == 0.0
        p, v, _ = ens.particles()
    ones = [np.ones(n, np.uint32) for n in sizes]
    rp, rv = _oracle_steps(orc, pos, vel, ones, 2)
    _assert_worlds_equal(p, rp, "weight None positions")
    _assert_worlds_equal(v, rv, "weight None velocities")
