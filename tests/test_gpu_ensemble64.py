"""Ensembles in f64 on the device (nb.Ensemble64 over nbody_ensemble64_*): every world of every test is compared body by body —
EXACT and AUTO with the oracle's update_direct of that world alone on float64, bit for bit; FAST with the contract of DESIGN §5,
|a - a_ref|_1 <= 1e-12 * sum_j |term_ij|_1 per body.  Needs an MI355X.

Sizes: the f32 file's (1, 2, 63 / 64 / 65 — also either side of a term block of 8 —, 257, 1000, 4096) and the boundaries of this
kernel's own layout table: 128 | 129 (two lanes per target | one target per lane), 256 | 257 (one | two blocks per world), 3272 |
3273 (the padded world is 65 440 | 65 600 bytes of LDS: above 64 KB the function's dynamic-LDS limit has to be raised), and for
FAST every lane split 4 | 5, 8 | 9, 16 | 17, 32 | 33, 64 | 65."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
FAST_RTOL = 1e-12   # the FAST f64 contract
HERE = os.path.dirname(os.path.abspath(__file__))


def _same_bits(a, b):
    """Equal as 64-bit integers — but for elements that are NaN on both sides: which payload an addition hands on is the one
    thing IEEE 754 leaves to the implementation (tests/test_gpu_ensemble.py does the same)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != F64 or b.dtype != F64:
        return False
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def _ties_rows():
    d = os.path.join(HERE, "golden", "reference_inputs", "c_signs_ties_wrap")
    pos = np.fromfile(os.path.join(d, "pos0.f32"), "<f4").reshape(-1, 2).astype(F64)
    vel = np.fromfile(os.path.join(d, "vel0.f32"), "<f4").reshape(-1, 2).astype(F64)
    return pos, vel, np.fromfile(os.path.join(d, "weight.u32"), "<u4")


def _uneven_weights(n, seed):
    """tests/test_gpu_direct_f64.py's weights, restated: odd values above 2^24 and values near the u32 wrap — a mass that passed
    through f32 on its way shows in the bits."""
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 1000, n).astype(np.uint32)
    w[::5] = (1 << 24) + 1 + 2 * np.arange(len(w[::5]), dtype=np.uint32)
    w[1::7] = np.uint32(0xFFFFFFFF) - np.arange(len(w[1::7]), dtype=np.uint32)
    return w


def _awkward_world(n):
    """Rows of c_signs_ties_wrap widened to double (both signs, a half-integer lattice, masses of 2^31 - 1; repeated past its 3000
    rows, which makes coincident points) with hand-made rows among them: +0 / -0, a 2^-1060 difference, the smallest normal, a
    coincident pair, an inf, a NaN, and 1.5e308 coordinates whose sums overflow."""
    pos, vel, w = _ties_rows()
    idx = np.arange(n) % pos.shape[0]
    idx[: min(n, 4)] = np.arange(0, 4 * 97, 97)[: min(n, 4)]          # the heavy rows first, so that every size has some
    p, v, w = pos[idx].copy(), vel[idx].copy(), w[idx].copy()
    tiny = np.ldexp(1.0, -1022)
    hand = np.array([[0.0, 0.0], [-0.0, 0.0], [np.ldexp(1.0, -1060), -0.0], [0.0, -tiny], [5.0, 5.0], [5.0, 5.0], [np.inf, 1.0],
                     [np.nan, 2.0], [1.5e308, 1.5e308], [-1.0e308, 1.7e308]], F64)
    if n >= 63:
        p[20:30] = hand
        w[22] = 0x7FFFFFFF
    elif n == 2:
        p[:] = [[0.0, -0.0], [-0.0, np.ldexp(1.0, -1060)]]
    return p, v, w


def _worlds(nb, n, b, seed, awkward_at=0):
    """b worlds of n bodies from distinct seeds (f64 Plummer sets with uneven weights); world `awkward_at` is _awkward_world(n)."""
    ps, vs, ws = [], [], []
    for k in range(b):
        if k == awkward_at:
            p, v, w = _awkward_world(n)
        else:
            p, v, _ = nb.scenes.plummer(n, seed=seed + k, dtype=F64)
            w = _uneven_weights(n, seed + k)
        ps.append(p), vs.append(v), ws.append(w)
    pos, vel = np.stack(ps), np.stack(vs)
    assert pos.dtype == F64 and vel.dtype == F64
    return pos, vel, np.stack(ws)


def _oracle_steps(orc, pos, vel, w, steps, clamp=0.001, delta=0.1):
    out = [orc.update_direct(pos[k], vel[k], w[k], delta=delta, clamp=clamp, nsteps=steps, nthreads=16)[:2] for k in range(pos.shape[0])]
    assert out[0][0].dtype == F64
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _assert_worlds_equal(got, want, what):
    assert got.dtype == F64 and got.shape == want.shape, what
    for k in range(want.shape[0]):
        assert _same_bits(got[k], want[k]), f"{what}: world {k} differs in {int((got[k].view(np.uint64) != want[k].view(np.uint64)).sum())} words"


def _fast_error(acc, ref, norm):
    """max_i |a - a_ref|_1 / sum_j |term_ij|_1"""
    return float((np.abs(acc - ref).sum(axis=1) / np.maximum(norm, 1e-300)).max())


# ------------------------------------------------------------------ 1. EXACT and AUTO, bit for bit
@pytest.mark.parametrize("arith,n", [("exact", n) for n in (1, 2, 63, 64, 65, 128, 129, 256, 257, 1000, 3272, 3273, 4096)]
                         + [("auto", n) for n in (1, 2, 63, 64, 65, 257, 1000, 4096)])
def test_exact_and_auto_every_world_bit_identical_to_its_oracle(nb, orc, arith, n):
    b = 2 if n >= 3000 else 5
    pos, vel, w = _worlds(nb, n, b, seed=100 + n, awkward_at=1)
    with nb.Ensemble64(pos, vel, w, arith=arith) as ens:
        assert ens.shape == (b, n)
        ens.update(0.1, None, n_steps=3)
        p, v, w2 = ens.particles()
        rp, rv = _oracle_steps(orc, pos, vel, w, 3)
        _assert_worlds_equal(p, rp, "positions")
        _assert_worlds_equal(v, rv, "velocities")
        assert np.array_equal(w2, w)
        acc = ens.accel()
        assert acc.dtype == F64
        for k in range(b):
            ref, _ = orc.direct_accel(rp[k], w[k], accum="native", nthreads=16)
            assert _same_bits(acc[k], ref), k
        p2, v2, _ = ens.particles()                       # accel() left the state's bytes alone
        assert p2.tobytes() == p.tobytes() and v2.tobytes() == v.tobytes()
    assert not np.array_equal(p[0], pos[0])               # (and something moved)


# ------------------------------------------------------------------ 2. a long run
def test_twenty_steps_of_the_ties_and_wraps_case_beside_a_plummer_world(nb, orc):
    n = 3000
    tp, tv, tw = _ties_rows()
    assert tp.shape[0] == n
    pp, pv, _ = nb.scenes.plummer(n, seed=0xE64, dtype=F64)
    pos, vel, w = np.stack([tp, pp]), np.stack([tv, pv]), np.stack([tw, _uneven_weights(n, 0xE64)])
    with nb.Ensemble64(pos, vel, w, arith="auto") as ens:
        ens.update(0.1, None, n_steps=20)
        p, v, _ = ens.particles()
    rp, rv = _oracle_steps(orc, pos, vel, w, 20)
    _assert_worlds_equal(p, rp, "positions after 20 steps")
    _assert_worlds_equal(v, rv, "velocities after 20 steps")


# ------------------------------------------------------------------ 3. FAST within 1e-12
@pytest.fixture(scope="module")
def galaxy(nb):
    return nb.scenes.galaxy(dtype=F64)


def _fast_worlds(nb, galaxy, n):
    """A Plummer world with uneven weights, a subset of the reference's scene that keeps its two heavy bodies, a world with close
    pairs under the clamp and one exact duplicate."""
    p0, v0, _ = nb.scenes.plummer(n, seed=300 + n, dtype=F64)
    w0 = _uneven_weights(n, 300 + n)
    gp, gv, gw = galaxy
    sel = np.concatenate([[0, 1], np.arange(2, gp.shape[0], max(1, (gp.shape[0] - 2) // n))])[:n]
    assert sel.shape[0] == n and gw[sel].max() > 10_000_000
    p2, v2, _ = nb.scenes.plummer(n, seed=400 + n, dtype=F64)
    w2 = (np.arange(n) % 3 + 1).astype(np.uint32)
    p2[1::8] = p2[0::8][: len(p2[1::8])] + 0.0078125             # d^2 = 6.1e-5 < 0.001
    if n > 40:
        p2[33] = p2[17]                                           # an exact duplicate
    pos = np.stack([p0, np.asarray(gp[sel], F64), p2])
    vel = np.stack([v0, np.asarray(gv[sel], F64), v2])
    assert pos.dtype == F64 and vel.dtype == F64
    return pos, vel, np.stack([w0, gw[sel].astype(np.uint32), w2])


@pytest.mark.parametrize("n", [64, 1000, 4096])
def test_fast_accel_within_1e12(nb, orc, galaxy, n):
    """Measured on an MI355X (max over the three worlds): 8.9e-16 at n = 64, 5.9e-15 at 1000, 1.3e-14 at 4096 (DESIGN §4.5′).
    The yardstick was checked on the CPU first: on these nine worlds the reference's own sequential chain (accum="native"), measured
    the same way against accum="f64", is finite everywhere and differs by 0.0 — in double both are the same chain of additions."""
    pos, vel, w = _fast_worlds(nb, galaxy, n)
    with nb.Ensemble64(pos, vel, w, arith="fast") as ens:
        acc = ens.accel()
        again = ens.accel()
    assert acc.tobytes() == again.tobytes()
    worst = 0.0
    for k in range(3):
        ref, norm = orc.direct_accel(pos[k], w[k], accum="f64", nthreads=16)
        assert np.all(np.isfinite(acc[k])), k
        r = _fast_error(acc[k], ref, norm)
        print(f"[tol] f64 ensemble FAST n={n} world {k}: max {r:.2e}")
        worst = max(worst, r)
        assert r <= FAST_RTOL, (n, k, r)
    print(f"[tol] f64 ensemble FAST n={n}: max over worlds {worst:.2e}")
    if n > 64:
        native, _ = orc.direct_accel(pos[0], w[0], accum="native", nthreads=16)
        assert not _same_bits(acc[0], native)                     # i.e. FAST really ran


# ------------------------------------------------------------------ 4. every layout
def test_fast_every_lane_split(nb, orc):
    """Sizes inside and at both ends of every range of ensemble_split (64, 32, 16, 8, 4, 2 lanes per target, one target per lane
    with one and with two blocks per world), odd and even: lanes past the end of a world store nothing, FAST reads no padding."""
    for n in (1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 24, 32, 33, 50, 64, 65, 100, 128, 129, 256, 257, 300):
        pos, vel, w = _worlds(nb, n, 3, seed=500 + n, awkward_at=-1)
        with nb.Ensemble64(pos, vel, w, arith="fast") as ens:
            acc = ens.accel()
            p, v, _ = ens.particles()
        assert p.tobytes() == pos.tobytes() and v.tobytes() == vel.tobytes()
        for k in range(3):
            ref, norm = orc.direct_accel(pos[k], w[k], accum="f64", nthreads=4)
            r = _fast_error(acc[k], ref, norm)
            assert np.all(np.isfinite(acc[k])) and r <= FAST_RTOL, (n, k, r)


# ------------------------------------------------------------------ 5. independence
@pytest.mark.parametrize("arith", ["fast", "exact"])
def test_a_world_depends_on_nothing_but_itself(nb, arith):
    n, b = 300, 7
    pos, vel, w = _worlds(nb, n, b, seed=700, awkward_at=3)      # (under FAST world 3 routes to EXACT, its neighbours do not)

    def run(p, v, ww):
        with nb.Ensemble64(p, v, ww, arith=arith) as ens:
            ens.update(0.1, None, n_steps=3)
            return ens.particles()[:2]

    p7, v7 = run(pos, vel, w)
    pr, vr = run(pos[::-1], vel[::-1], w[::-1])
    for k in range(b):
        p1, v1 = run(pos[k:k + 1], vel[k:k + 1], w[k:k + 1])
        assert _same_bits(p7[k], p1[0]) and _same_bits(v7[k], v1[0]), k
        assert _same_bits(p7[k], pr[b - 1 - k]) and _same_bits(v7[k], vr[b - 1 - k]), k
        assert not np.array_equal(p7[k], pos[k])


# ------------------------------------------------------------------ 6. FAST routes per world
def _outside_domain(x):
    x = abs(float(x))
    return not (x < 2.0 ** 100) or 0.0 < x < 2.0 ** -300


def _routed_worlds(nb, poison):
    """Three worlds of 200; body 7 of world 1 is at rest at (poison, 3.0).
    inf stays inf, and 2^100 absorbs whatever a step adds to it.  A coordinate of 1e-305 is another matter in double: the pull of
    a Plummer world (~1e-8) would carry it to ~1e-10, inside the domain, within one step.  So for that poison world 1 is mirrored
    in x: its other bodies come as neighbours in j (x, y), (-x, y) of equal weight, whose terms on body 7 are exact opposites
    (x - 1e-305 rounds to x) and cancel pair by pair in the ascending chain, plus one body on the axis x = 0, whose term is
    subnormal.  The oracle confirms below that the coordinate stays under 2^-300."""
    n = 200
    pos, vel, w = _worlds(nb, n, 3, seed=800, awkward_at=-1)
    if 0.0 < poison < 1.0:
        half, hv, _ = nb.scenes.plummer(99, seed=877, dtype=F64)
        hw = _uneven_weights(99, 877)
        others = [k for k in range(n) if k != 7]
        for m in range(99):
            a, b = others[2 * m], others[2 * m + 1]
            pos[1, a], pos[1, b] = half[m], half[m] * (-1.0, 1.0)
            vel[1, a], vel[1, b] = hv[m], hv[m] * (-1.0, 1.0)
            w[1, a] = w[1, b] = hw[m]
        pos[1, others[198]] = (0.0, 12345.0)
        vel[1, others[198]] = (0.0, 0.25)
    pos[1, 7] = (poison, 3.0)
    vel[1, 7] = (0.0, 0.0)
    return pos, vel, w


@pytest.mark.parametrize("poison", [1e-305, np.inf, 2.0 ** 100])
def test_fast_routes_each_world_on_its_own(nb, orc, poison):
    pos, vel, w = _routed_worlds(nb, poison)
    assert _outside_domain(pos[1, 7, 0])
    rp1, _ = _oracle_steps(orc, pos, vel, w, 1)
    assert _outside_domain(rp1[1, 7, 0]), rp1[1, 7, 0]           # still outside when the second step starts
    rp, rv = _oracle_steps(orc, pos, vel, w, 2)
    assert _outside_domain(rp[1, 7, 0]), rp[1, 7, 0]             # ... and when accel() below looks
    for k in (0, 2):
        assert not any(_outside_domain(x) for x in rp1[k].ravel()) and not any(_outside_domain(x) for x in rp[k].ravel())
    with nb.Ensemble64(pos, vel, w, arith="fast") as ens:
        ens.update(0.1, None, n_steps=2)
        pa, va, _ = ens.particles()
        acc = ens.accel()
    with nb.Ensemble64(pos[[0, 2]], vel[[0, 2]], w[[0, 2]], arith="fast") as ens:
        ens.update(0.1, None, n_steps=2)
        pf, vf, _ = ens.particles()
    assert _same_bits(pa[1], rp[1]) and _same_bits(va[1], rv[1])
    for k, kf in ((0, 0), (2, 1)):
        assert _same_bits(pa[k], pf[kf]) and _same_bits(va[k], vf[kf]), k
    # the routes themselves, in the accelerations of the third step: world 1 EXACT, its neighbours not
    for k in range(3):
        ref, _ = orc.direct_accel(pa[k], w[k], accum="native", nthreads=16)
        assert _same_bits(acc[k], ref) == (k == 1), k
    # a clamp that is not > 0: every world EXACT
    rp, rv = _oracle_steps(orc, pos, vel, w, 2, clamp=0.0)
    with nb.Ensemble64(pos, vel, w, arith="fast", clamp=0.0) as ens:
        ens.update(0.1, None, n_steps=2)
        pa, va, _ = ens.particles()
    _assert_worlds_equal(pa, rp, "clamp 0 positions")
    _assert_worlds_equal(va, rv, "clamp 0 velocities")


# ------------------------------------------------------------------ 7. buffers
@pytest.mark.parametrize("arith", ["fast", "exact"])
def test_steps_split_over_calls_and_a_second_upload(nb, orc, arith):
    pos, vel, w = _worlds(nb, 257, 3, seed=600, awkward_at=-1)
    with nb.Ensemble64(pos, vel, w, arith=arith) as ens:
        ens.update(0.1, None, n_steps=5)                         # an odd count: ends on the other buffer
        p5, v5, _ = ens.particles()
        ens.upload(pos, vel, w)
        for _ in range(5):
            ens.update(0.1, None, n_steps=1)
            p1, v1, _ = ens.particles()
        ens.upload(pos, vel, w)
        ens.update(0.1, None, n_steps=2)                         # an even count
        p2, v2, _ = ens.particles()
        ens.update(0.1, None, n_steps=3)
        p23, v23, _ = ens.particles()
        assert p5.tobytes() == p1.tobytes() == p23.tobytes() and v5.tobytes() == v1.tobytes() == v23.tobytes()
        assert p2.tobytes() != p5.tobytes()
        if arith == "exact":
            rp, rv = _oracle_steps(orc, pos, vel, w, 5)
            _assert_worlds_equal(p5, rp, "5 steps")
            _assert_worlds_equal(v5, rv, "5 steps")
            rp, rv = _oracle_steps(orc, pos, vel, w, 2)
            _assert_worlds_equal(p2, rp, "2 steps")
            _assert_worlds_equal(v2, rv, "2 steps")
        # another shape on the same handle
        pos, vel, w = _worlds(nb, 65, 2, seed=650, awkward_at=0)
        ens.upload(pos, vel, w)
        assert ens.shape == (2, 65)
        ens.h.set_params(arith=nb._capi.ARITH_EXACT)
        ens.update(0.1, None, n_steps=3)
        p, v, w2 = ens.particles()
        rp, rv = _oracle_steps(orc, pos, vel, w, 3)
        _assert_worlds_equal(p, rp, "second upload")
        _assert_worlds_equal(v, rv, "second upload")
        assert np.array_equal(w2, w)


# ------------------------------------------------------------------ 8. call order and coexistence
def test_call_order_and_other_handles_beside_the_ensemble(nb, orc):
    C = nb._capi
    h = C.Ensemble64Handle(0)
    try:
        assert h.shape == (0, 0)
        for call in (lambda: h.update(0.1, 1), lambda: h.update(0.1, 0), h.accel, h.download):
            with pytest.raises(C.NBodyError) as e:
                call()
            assert e.value.code == C.ERR_INVALID and "ensemble" in str(e.value)
        with pytest.raises(C.NBodyError) as e:
            h.upload(1, 4097, np.zeros((4097, 2), F64), np.zeros((4097, 2), F64), None)
        assert e.value.code == C.ERR_INVALID and "ensemble" in str(e.value) and h.shape == (0, 0)
    finally:
        h.close()

    pos, vel, w = _worlds(nb, 200, 3, seed=750, awkward_at=-1)
    cnt = nb.Counting()
    with nb.Ensemble64(pos, vel, w, arith="auto") as ens:
        ens.update(0.1, cnt, n_steps=0)
        p, v, _ = ens.particles()
        assert p.tobytes() == pos.tobytes() and v.tobytes() == vel.tobytes() and cnt.sum_gravity == 0.0
        with pytest.raises(C.NBodyError):
            ens.update(0.1, None, n_steps=-1)
        ens.update(0.1, cnt, n_steps=2)
        assert cnt.sum_gravity > 0.0 and cnt.build_bvh == 0.0 and cnt.post_calculations == 0.0

    # weight None is all 1
    with nb.Ensemble64(pos, vel, None, arith="exact") as ens:
        ens.update(0.1, None, n_steps=1)
        p, v, w1 = ens.particles()
    ones = np.ones(w.shape, np.uint32)
    rp, rv = _oracle_steps(orc, pos, vel, ones, 1)
    _assert_worlds_equal(p, rp, "weight None")
    assert np.array_equal(w1, ones)

    p32, v32 = pos.astype(F32), vel.astype(F32)
    w32 = (w % 11 + 1).astype(np.uint32)

    def others(between=None):
        """An f32 ensemble and an f64 direct World, three calls each, `between` after every one of them."""
        world = nb.World(pos[0], vel[0], w[0], method="direct", arith="exact")
        try:
            with nb.Ensemble(p32, v32, w32, arith="fast") as e32:
                for _ in range(3):
                    world.update(0.1, None, n_steps=2)
                    if between:
                        between()
                    e32.update(0.1, None, n_steps=1)
                    if between:
                        between()
                pe, ve, _ = e32.particles()
            pw, vw = world.particles()[:2]
            return pe.tobytes(), ve.tobytes(), pw.tobytes(), vw.tobytes()
        finally:
            world.close()

    alone = others()
    with nb.Ensemble64(pos, vel, w, arith="fast") as ens:
        beside = others(lambda: ens.update(0.1, None, n_steps=1))
        p64, v64, _ = ens.particles()
    assert alone == beside
    with nb.Ensemble64(pos, vel, w, arith="fast") as ens:        # and the f64 ensemble did not notice them either
        ens.update(0.1, None, n_steps=6)
        pq, vq, _ = ens.particles()
    assert pq.tobytes() == p64.tobytes() and vq.tobytes() == v64.tobytes()
