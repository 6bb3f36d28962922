"""Ragged ensembles on the device (nb.RaggedEnsemble over nbody_ragged_*): worlds of different sizes stepped together.  Every
world is compared on its own — EXACT with the oracle's update_direct of that world alone, bit for bit; FAST with nb.Ensemble
holding that world alone, bit for bit (the two kernels share one body), and with the frozen tolerance of tests/_tol.py.  Needs an
MI355X.

Sizes: odd ones early, so that later worlds start at odd rows; 128 / 129 and 256 / 257 on either side of a lane split and of a
launch class; one size inside every range of ensemble_split; 4096, the top size (16 blocks, 48 KB of LDS)."""
import os

import numpy as np
import pytest

from tests._tol import ACC_RTOL, check_fast

pytestmark = pytest.mark.gpu
F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))

MIXED = [300, 1, 65, 4096, 2, 257, 63, 128, 129, 1000, 7, 64, 256]
EVERY_SPLIT = (1, 2, 3, 7, 12, 24, 50, 100, 128, 129, 256, 257, 300, 1000, 4096)


def _same_bits(a, b):
    """Equal as integers — but for elements that are NaN on both sides: which payload an addition hands on is the one thing
    IEEE 754 leaves to the implementation."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _ties_rows():
    d = os.path.join(HERE, "golden", "reference_inputs", "c_signs_ties_wrap")
    pos = np.fromfile(os.path.join(d, "pos0.f32"), "<f4").reshape(-1, 2)
    vel = np.fromfile(os.path.join(d, "vel0.f32"), "<f4").reshape(-1, 2)
    return pos, vel, np.fromfile(os.path.join(d, "weight.u32"), "<u4")


def _awkward_world(n):
    """Rows of c_signs_ties_wrap (both signs, a half-integer lattice, masses of 2^31 - 1) with hand-made rows among them: +0 / -0,
    subnormal differences, a coincident pair, an inf, a NaN."""
    pos, vel, w = _ties_rows()
    idx = np.arange(n) % pos.shape[0]
    idx[: min(n, 4)] = np.arange(0, 4 * 97, 97)[: min(n, 4)]
    p, v, w = pos[idx].copy(), vel[idx].copy(), w[idx].copy()
    hand = np.array([[0.0, 0.0], [-0.0, 0.0], [1e-39, -0.0], [0.0, -1e-40], [5.0, 5.0], [5.0, 5.0], [np.inf, 1.0], [np.nan, 2.0]], F32)
    if n >= 63:
        p[20:28] = hand
        w[22] = 0x7FFFFFFF
    elif n == 2:
        p[:] = [[0.0, -0.0], [-0.0, 1e-39]]
    return p.astype(F32), v.astype(F32), w


def _worlds(nb, sizes, seed, awkward_at=()):
    """One world per size from distinct seeds (Plummer sets with mixed masses); the worlds at `awkward_at` are _awkward_world."""
    ps, vs, ws = [], [], []
    for k, n in enumerate(sizes):
        if k in awkward_at:
            p, v, w = _awkward_world(n)
        else:
            p, v, _ = nb.scenes.plummer(n, seed=seed + k)
            w = ((np.arange(n) * (k + 3)) % 11 + 1).astype(np.uint32)
        ps.append(np.ascontiguousarray(p, F32)), vs.append(np.ascontiguousarray(v, F32)), ws.append(w)
    return ps, vs, ws


def _oracle_steps(orc, pos, vel, w, steps, clamp=0.001, delta=0.1):
    out = [orc.update_direct(pos[k], vel[k], w[k], delta=delta, clamp=clamp, nsteps=steps, nthreads=16)[:2] for k in range(len(pos))]
    return [o[0] for o in out], [o[1] for o in out]


def _assert_worlds_equal(got, want, what):
    assert len(got) == len(want), what
    for k in range(len(want)):
        assert _same_bits(got[k], want[k]), f"{what}: world {k} (n = {len(want[k])}) differs"


def _ragged_run(nb, pos, vel, w, arith, steps, clamp=0.001):
    with nb.RaggedEnsemble(pos, vel, w, arith=arith, clamp=clamp) as ens:
        ens.update(0.1, None, n_steps=steps)
        p, v, _ = ens.particles()
        return p, v, ens.accel()


def _uniform_run(nb, p, v, w, arith, steps):
    """nb.Ensemble holding this one world -> its positions, velocities after `steps` steps and the accelerations there."""
    with nb.Ensemble(p[None], v[None], w[None], arith=arith) as ens:
        ens.update(0.1, None, n_steps=steps)
        pp, vv, _ = ens.particles()
        return pp[0], vv[0], ens.accel()[0]


# ------------------------------------------------------------------ 1. EXACT, mixed sizes
def test_exact_mixed_sizes_every_world_bit_identical_to_its_oracle(nb, orc):
    pos, vel, w = _worlds(nb, MIXED, seed=1100, awkward_at=(5,))
    with nb.RaggedEnsemble(pos, vel, w, arith="exact") as ens:
        assert ens.sizes == MIXED and ens.h.shape == (len(MIXED), sum(MIXED)) and ens.h.sizes.tolist() == MIXED
        ens.update(0.1, None, n_steps=3)
        p, v, w2 = ens.particles()
        assert [a.shape for a in p] == [(n, 2) for n in MIXED] and [a.shape for a in w2] == [(n,) for n in MIXED]
        rp, rv = _oracle_steps(orc, pos, vel, w, 3)
        _assert_worlds_equal(p, rp, "positions")
        _assert_worlds_equal(v, rv, "velocities")
        assert all(np.array_equal(a, b) for a, b in zip(w2, w))
        acc = ens.accel()
        for k in range(len(MIXED)):
            ref, _ = orc.direct_accel(rp[k], w[k], nthreads=16)
            assert _same_bits(acc[k], ref.astype(F32)), k
        p2, v2, _ = ens.particles()                       # accel() left the state's bits alone
        assert all(a.tobytes() == b.tobytes() for a, b in zip(p2 + v2, p + v))


# ------------------------------------------------------------------ 2. FAST equals the uniform ensemble, bit for bit
def test_fast_every_world_bit_identical_to_the_uniform_ensemble(nb, orc):
    sizes = list(EVERY_SPLIT)
    pos, vel, w = _worlds(nb, sizes, seed=1200)
    p, v, acc = _ragged_run(nb, pos, vel, w, "fast", 3)
    for k, n in enumerate(sizes):
        up, uv, ua = _uniform_run(nb, pos[k], vel[k], w[k], "fast", 3)
        assert _same_bits(p[k], up) and _same_bits(v[k], uv), f"n = {n}: state differs from nb.Ensemble of that world alone"
        assert _same_bits(acc[k], ua), f"n = {n}: accel differs from nb.Ensemble of that world alone"
        assert n == 1 or not np.array_equal(p[k], pos[k]), n


@pytest.fixture(scope="module")
def galaxy(nb):
    return nb.scenes.galaxy()


def _fast_worlds(nb, galaxy, n):
    """A Plummer world, a subset of the reference's scene that keeps its two heavy bodies, a world with close pairs under the clamp."""
    p0, v0, _ = nb.scenes.plummer(n, seed=300 + n)
    w0 = (np.arange(n) % 5 + 1).astype(np.uint32)
    gp, gv, gw = galaxy
    sel = np.concatenate([[0, 1], np.arange(2, gp.shape[0], max(1, (gp.shape[0] - 2) // n))])[:n]
    assert sel.shape[0] == n and gw[sel].max() > 10_000_000
    p2, v2, _ = nb.scenes.plummer(n, seed=400 + n)
    w2 = (np.arange(n) % 3 + 1).astype(np.uint32)
    p2[1::8] = p2[0::8][: len(p2[1::8])] + F32(0.0078125)        # d^2 = 6.1e-5 < 0.001
    if n > 40:
        p2[33] = p2[17]                                           # an exact duplicate
    return ([a.astype(F32) for a in (p0, gp[sel], p2)], [a.astype(F32) for a in (v0, gv[sel], v2)], [w0, gw[sel], w2])


def test_fast_accel_within_the_frozen_tolerance(nb, orc, galaxy):
    pos, vel, w, sizes = [], [], [], []
    for n in (64, 1000, 4096):                                    # interleaved below: 64, 1000, 4096, 64, 1000, ...
        p, v, ww = _fast_worlds(nb, galaxy, n)
        pos.append(p), vel.append(v), w.append(ww)
    pos, vel, w = ([x[i][j] for j in range(3) for i in range(3)] for x in (pos, vel, w))
    sizes = [len(p) for p in pos]
    assert sizes == [64, 1000, 4096] * 3
    with nb.RaggedEnsemble(pos, vel, w, arith="fast") as ens:
        acc = ens.accel()
    assert ACC_RTOL == 2e-5
    for k, n in enumerate(sizes):
        ref64, norm = orc.direct_accel(pos[k], w[k], accum="f64", nthreads=16)
        cpu32, _ = orc.direct_accel(pos[k], w[k], nthreads=16)
        check_fast(acc[k], ref64, norm, cpu32, label=f" n={n} world {k}")
        if n > 64 and k < 3:
            assert not np.array_equal(acc[k], cpu32.astype(F32)), n   # i.e. FAST really ran


# ------------------------------------------------------------------ 3. equal sizes through the ragged route
@pytest.mark.parametrize("arith", ["fast", "exact"])
def test_equal_sizes_through_the_ragged_kernel_equal_the_uniform_ensemble(nb, arith):
    pos, vel, w = _worlds(nb, [300] * 5, seed=1300, awkward_at=(1,))
    p, v, acc = _ragged_run(nb, pos, vel, w, arith, 5)
    with nb.Ensemble(np.stack(pos), np.stack(vel), np.stack(w), arith=arith) as ens:
        ens.update(0.1, None, n_steps=5)
        up, uv, _ = ens.particles()
        ua = ens.accel()
    _assert_worlds_equal(p, list(up), "positions")
    _assert_worlds_equal(v, list(uv), "velocities")
    _assert_worlds_equal(acc, list(ua), "accel")
    assert not np.array_equal(p[0], pos[0])


# ------------------------------------------------------------------ 4. independence
@pytest.mark.parametrize("arith", ["fast", "auto"])
def test_a_world_depends_on_nothing_but_itself(nb, arith):
    sizes = [300, 7, 129, 300, 64, 1000, 2, 128]
    pos, vel, w = _worlds(nb, sizes, seed=1400, awkward_at=(3,))   # (under AUTO world 3 routes to EXACT, its neighbours do not)
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
    # neighbours of another size: world 2 grows from 129 to 4096 (another launch class, 16 blocks where there was one), world 4
    # from 64 to 65 (another lane split, and with it another LDS for the launch it shares with worlds 1, 6 and 7); every row
    # after them shifts
    pos2, vel2, w2 = list(pos), list(vel), list(w)
    for k, n in ((2, 4096), (4, 65)):
        pk, vk, wk = _worlds(nb, [n], seed=1460 + k)
        pos2[k], vel2[k], w2[k] = pk[0], vk[0], wk[0]
    pn, vn, _ = _ragged_run(nb, pos2, vel2, w2, arith, 3)
    for k in range(b):
        if k not in (2, 4):
            assert _same_bits(p0[k], pn[k]) and _same_bits(v0[k], vn[k]), k
        if arith == "fast" or k != 3:
            assert not np.array_equal(p0[k], pos[k])


@pytest.mark.parametrize("poison", [1e-30, np.inf])
def test_auto_routes_each_world_on_its_own(nb, orc, poison):
    sizes = [200, 150, 200, 1000, 50, 256, 200]        # world 2 is poisoned: 0, 1, 5, 6 share its launch class, 3 and 4 do not
    pos, vel, w = _worlds(nb, sizes, seed=1500)
    # the poisoned body sits far from its world (Plummer sets around (50000, 50000)) and at rest: its acceleration is ~1e-8, so
    # after a step the coordinate is still non-zero below 2^-22 and the world is still outside FAST's domain (checked below)
    pos[2][7] = (poison, 3.0)
    vel[2][7] = (0.0, 0.0)
    rp1, _ = _oracle_steps(orc, pos[2:3], vel[2:3], w[2:3], 1)
    x = abs(float(rp1[0][7, 0]))
    assert not (x < 2.0 ** 60) or 0.0 < x < 2.0 ** -22
    rp, rv = _oracle_steps(orc, pos, vel, w, 2)
    pa, va, acc = _ragged_run(nb, pos, vel, w, "auto", 2)
    pf, vf, _ = _ragged_run(nb, pos, vel, w, "fast", 2)
    assert _same_bits(pa[2], rp[2]) and _same_bits(va[2], rv[2])
    for k in range(len(sizes)):
        if k != 2:
            assert _same_bits(pa[k], pf[k]) and _same_bits(va[k], vf[k]), k
    # the routes themselves, in the accelerations of the third step: world 2 EXACT, the others not
    for k in range(len(sizes)):
        ref, _ = orc.direct_accel(pa[k], w[k], nthreads=16)
        assert _same_bits(acc[k], ref.astype(F32)) == (k == 2), k
    # a clamp below FAST's floor: every world EXACT
    rp, rv = _oracle_steps(orc, pos, vel, w, 2, clamp=1e-7)
    pa, va, _ = _ragged_run(nb, pos, vel, w, "auto", 2, clamp=1e-7)
    _assert_worlds_equal(pa, rp, "clamp 1e-7 positions")
    _assert_worlds_equal(va, rv, "clamp 1e-7 velocities")


# ------------------------------------------------------------------ 5. buffers and call order
@pytest.mark.parametrize("arith", ["fast", "exact"])
def test_steps_split_over_calls_and_a_second_upload(nb, orc, arith):
    sizes = [257, 3, 129, 64]
    pos, vel, w = _worlds(nb, sizes, seed=1600)

    def state(ens):
        p, v, _ = ens.particles()
        return b"".join(a.tobytes() for a in p + v)

    with nb.RaggedEnsemble(pos, vel, w, arith=arith) as ens:
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
        pos, vel, w = _worlds(nb, sizes2, seed=1650, awkward_at=(0,))
        ens.upload(pos, vel, w)
        assert ens.sizes == sizes2 and ens.h.shape == (5, sum(sizes2))
        ens.h.set_params(arith=nb._capi.ARITH_EXACT)
        ens.update(0.1, None, n_steps=3)
        p, v, w2 = ens.particles()
        rp, rv = _oracle_steps(orc, pos, vel, w, 3)
        _assert_worlds_equal(p, rp, "second upload")
        _assert_worlds_equal(v, rv, "second upload")
        assert all(np.array_equal(a, b) for a, b in zip(w2, w))


def test_call_order_and_booking(nb):
    C = nb._capi
    h = C.RaggedHandle(0)
    try:
        assert h.shape == (0, 0) and h.sizes.tolist() == []
        for call in (lambda: h.update(0.1, 1), lambda: h.update(0.1, 0), h.accel, h.download):
            with pytest.raises(C.NBodyError) as e:
                call()
            assert e.value.code == C.ERR_INVALID and "ragged" in str(e.value)
        for bad in ([4, 4097], [0, 4], []):
            n = max(sum(bad), 1)
            with pytest.raises(C.NBodyError) as e:
                h.upload(np.array(bad, np.int64), np.zeros((n, 2), F32), np.zeros((n, 2), F32), None)
            assert e.value.code == C.ERR_INVALID and "ragged" in str(e.value) and h.shape == (0, 0)
    finally:
        h.close()

    sizes = [200, 9, 600]
    pos, vel, w = _worlds(nb, sizes, seed=1700)
    cnt = nb.Counting()
    with nb.RaggedEnsemble(pos, vel, None, arith="auto") as ens:      # no weights: all 1
        ens.update(0.1, cnt, n_steps=0)
        p, v, w1 = ens.particles()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(p + v, pos + vel)) and cnt.sum_gravity == 0.0
        assert all(a.dtype == np.uint32 and (a == 1).all() for a in w1)
        with pytest.raises(C.NBodyError):
            ens.update(0.1, None, n_steps=-1)
        ens.update(0.1, cnt, n_steps=2)
        assert cnt.sum_gravity > 0.0 and cnt.build_bvh == 0.0 and cnt.post_calculations == 0.0
        p, _, _ = ens.particles()
    ones = [np.ones(n, np.uint32) for n in sizes]
    p1, _, _ = _ragged_run(nb, pos, vel, ones, "auto", 2)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(p, p1))
