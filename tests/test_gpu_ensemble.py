"""Ensembles on the device (nb.Ensemble over nbody_ensemble_*): every world of every test is compared body by body — EXACT with
the oracle's update_direct of that world alone, bit for bit; FAST with the frozen tolerance of tests/_tol.py.  Needs an MI355X.

Sizes: 1, 2 (64 lanes per target), 63 / 64 (4 lanes), 65 (2 lanes), 257 / 300 (one target per lane, a second block with a few
live lanes), 1000, 4096 (the top size: 48 KB of LDS, 16 blocks per world); test_fast_every_lane_split adds the splits between."""
import os

import numpy as np
import pytest

from tests._tol import ACC_RTOL, check_fast

pytestmark = pytest.mark.gpu
F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "config1_1024.npz"))


def _same_bits(a, b):
    """Equal as integers — but for elements that are NaN on both sides: which payload an addition hands on is the one thing
    IEEE 754 leaves to the implementation (the other EXACT tests compare such rows with equal_nan for the same reason)."""
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
    """Rows of c_signs_ties_wrap (both signs, a half-integer lattice, masses of 2^31 - 1; repeated past its 3000 rows, which makes
    coincident points) with hand-made rows among them: +0 / -0, subnormal differences, a coincident pair, an inf, a NaN."""
    pos, vel, w = _ties_rows()
    idx = np.arange(n) % pos.shape[0]
    idx[: min(n, 4)] = np.arange(0, 4 * 97, 97)[: min(n, 4)]          # the heavy rows first, so that every size has some
    p, v, w = pos[idx].copy(), vel[idx].copy(), w[idx].copy()
    hand = np.array([[0.0, 0.0], [-0.0, 0.0], [1e-39, -0.0], [0.0, -1e-40], [5.0, 5.0], [5.0, 5.0], [np.inf, 1.0], [np.nan, 2.0]], F32)
    if n >= 63:
        p[20:28] = hand
        w[22] = 0x7FFFFFFF
    elif n == 2:
        p[:] = [[0.0, -0.0], [-0.0, 1e-39]]
    return p, v, w


def _worlds(nb, n, b, seed, awkward_at=0):
    """b worlds of n bodies from distinct seeds (Plummer sets with mixed masses); world `awkward_at` is _awkward_world(n)."""
    ps, vs, ws = [], [], []
    for k in range(b):
        if k == awkward_at:
            p, v, w = _awkward_world(n)
        else:
            p, v, _ = nb.scenes.plummer(n, seed=seed + k)
            w = ((np.arange(n) * (k + 3)) % 11 + 1).astype(np.uint32)
        ps.append(p), vs.append(v), ws.append(w)
    return np.stack(ps).astype(F32), np.stack(vs).astype(F32), np.stack(ws)


def _oracle_steps(orc, pos, vel, w, steps, clamp=0.001, delta=0.1):
    out = [orc.update_direct(pos[k], vel[k], w[k], delta=delta, clamp=clamp, nsteps=steps, nthreads=16)[:2] for k in range(pos.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _assert_worlds_equal(got, want, what):
    for k in range(want.shape[0]):
        assert _same_bits(got[k], want[k]), f"{what}: world {k} differs in {int((got[k].view(np.uint32) != want[k].view(np.uint32)).sum())} words"


# ------------------------------------------------------------------ 1. EXACT, bit for bit
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1000, 4096])
def test_exact_every_world_bit_identical_to_its_oracle(nb, orc, n):
    b = 2 if n == 4096 else 5
    pos, vel, w = _worlds(nb, n, b, seed=100 + n, awkward_at=1)
    with nb.Ensemble(pos, vel, w, arith="exact") as ens:
        assert ens.shape == (b, n)
        ens.update(0.1, None, n_steps=3)
        p, v, w2 = ens.particles()
        rp, rv = _oracle_steps(orc, pos, vel, w, 3)
        _assert_worlds_equal(p, rp, "positions")
        _assert_worlds_equal(v, rv, "velocities")
        assert np.array_equal(w2, w)
        acc = ens.accel()
        for k in range(b):
            ref, _ = orc.direct_accel(rp[k], w[k], nthreads=16)
            assert _same_bits(acc[k], ref.astype(F32)), k
        p2, v2, _ = ens.particles()                       # accel() left the state's bits alone
        assert p2.tobytes() == p.tobytes() and v2.tobytes() == v.tobytes()


# ------------------------------------------------------------------ 2. the golden trajectory, as world 2 of 4
def test_golden_trajectory_as_one_world_among_four(nb):
    ps, vs, ws = [], [], []
    for k in range(4):
        if k == 2:
            p, v, w = G["ic_pos"], G["ic_vel"], G["ic_weight"]
        else:
            p, v, w = nb.scenes.plummer(1024, seed=900 + k)
        ps.append(p), vs.append(v), ws.append(w)
    with nb.Ensemble(np.stack(ps), np.stack(vs), np.stack(ws), arith="exact") as ens:
        ens.update(0.1, None, n_steps=100)
        p, v, _ = ens.particles()
    assert _same_bits(p[2], G["direct_s100_pos"]) and _same_bits(v[2], G["direct_s100_vel"])
    assert not np.array_equal(p[1], p[2])


# ------------------------------------------------------------------ 3. FAST within the frozen tolerance
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
    return (np.stack([p0, gp[sel], p2]).astype(F32), np.stack([v0, gv[sel], v2]).astype(F32), np.stack([w0, gw[sel], w2]))


@pytest.mark.parametrize("n", [64, 1000, 4096])
def test_fast_accel_within_the_frozen_tolerance(nb, orc, galaxy, n):
    pos, vel, w = _fast_worlds(nb, galaxy, n)
    with nb.Ensemble(pos, vel, w, arith="fast") as ens:
        acc = ens.accel()
    assert ACC_RTOL == 2e-5
    for k in range(3):
        ref64, norm = orc.direct_accel(pos[k], w[k], accum="f64", nthreads=16)
        cpu32, _ = orc.direct_accel(pos[k], w[k], nthreads=16)
        check_fast(acc[k], ref64, norm, cpu32, label=f" n={n} world {k}")
    ref, _ = orc.direct_accel(pos[0], w[0], nthreads=16)
    if n > 64:
        assert not np.array_equal(acc[0], ref.astype(F32))       # i.e. FAST really ran


def test_fast_every_lane_split(nb, orc):
    """One size inside every range of ensemble_split (64, 32, 16, 8, 4, 2 lanes per target, one target per lane with one and
    with two blocks per world), odd and even: the padded source of an odd world adds nothing, lanes past the end store nothing."""
    for n in (1, 2, 3, 7, 12, 24, 50, 100, 128, 129, 300):
        pos, vel, w = _worlds(nb, n, 3, seed=500 + n, awkward_at=-1)
        with nb.Ensemble(pos, vel, w, arith="fast") as ens:
            acc = ens.accel()
            p, v, _ = ens.particles()
        assert p.tobytes() == pos.tobytes() and v.tobytes() == vel.tobytes()
        for k in range(3):
            ref64, norm = orc.direct_accel(pos[k], w[k], accum="f64", nthreads=4)
            check_fast(acc[k], ref64, norm, label=f" n={n} world {k}")


# ------------------------------------------------------------------ 4. independence
@pytest.mark.parametrize("arith", ["fast", "auto"])
def test_a_world_depends_on_nothing_but_itself(nb, arith):
    n, b = 300, 7
    pos, vel, w = _worlds(nb, n, b, seed=700, awkward_at=3)      # (under AUTO world 3 routes to EXACT, its neighbours do not)

    def run(p, v, ww):
        with nb.Ensemble(p, v, ww, arith=arith) as ens:
            ens.update(0.1, None, n_steps=3)
            return ens.particles()[:2]

    p7, v7 = run(pos, vel, w)
    pr, vr = run(pos[::-1], vel[::-1], w[::-1])
    for k in range(b):
        p1, v1 = run(pos[k:k + 1], vel[k:k + 1], w[k:k + 1])
        assert _same_bits(p7[k], p1[0]) and _same_bits(v7[k], v1[0]), k
        assert _same_bits(p7[k], pr[b - 1 - k]) and _same_bits(v7[k], vr[b - 1 - k]), k
        if arith == "fast" or k != 3:
            assert not np.array_equal(p7[k], pos[k])


# ------------------------------------------------------------------ 5. AUTO routes per world
@pytest.mark.parametrize("poison", [1e-30, np.inf])
def test_auto_routes_each_world_on_its_own(nb, orc, poison):
    n = 200
    pos, vel, w = _worlds(nb, n, 3, seed=800, awkward_at=-1)
    # the poisoned body sits far from its world (Plummer sets around (50000, 50000)) and at rest: its acceleration is ~1e-8, so
    # after a step the coordinate is still non-zero below 2^-22 and the world is still outside FAST's domain (checked below)
    pos[1, 7] = (poison, 3.0)
    vel[1, 7] = (0.0, 0.0)
    rp1, _ = _oracle_steps(orc, pos, vel, w, 1)
    x = abs(float(rp1[1, 7, 0]))
    assert not (x < 2.0 ** 60) or 0.0 < x < 2.0 ** -22
    rp, rv = _oracle_steps(orc, pos, vel, w, 2)
    with nb.Ensemble(pos, vel, w, arith="auto") as ens:
        ens.update(0.1, None, n_steps=2)
        pa, va, _ = ens.particles()
        acc = ens.accel()
    with nb.Ensemble(pos, vel, w, arith="fast") as ens:
        ens.update(0.1, None, n_steps=2)
        pf, vf, _ = ens.particles()
    assert _same_bits(pa[1], rp[1]) and _same_bits(va[1], rv[1])
    for k in (0, 2):
        assert _same_bits(pa[k], pf[k]) and _same_bits(va[k], vf[k]), k
    # the routes themselves, in the accelerations of the third step (accelerations here are ~1e-8 of the velocities, so two
    # steps of FAST can leave the oracle's very bits in the state): world 1 EXACT, its neighbours not
    for k in range(3):
        ref, _ = orc.direct_accel(pa[k], w[k], nthreads=16)
        assert _same_bits(acc[k], ref.astype(F32)) == (k == 1), k
    # a clamp below FAST's floor: every world EXACT
    rp, rv = _oracle_steps(orc, pos, vel, w, 2, clamp=1e-7)
    with nb.Ensemble(pos, vel, w, arith="auto", clamp=1e-7) as ens:
        ens.update(0.1, None, n_steps=2)
        pa, va, _ = ens.particles()
    _assert_worlds_equal(pa, rp, "clamp 1e-7 positions")
    _assert_worlds_equal(va, rv, "clamp 1e-7 velocities")


# ------------------------------------------------------------------ 6. buffers
@pytest.mark.parametrize("arith", ["fast", "exact"])
def test_steps_split_over_calls_and_a_second_upload(nb, orc, arith):
    pos, vel, w = _worlds(nb, 257, 3, seed=600, awkward_at=-1)
    with nb.Ensemble(pos, vel, w, arith=arith) as ens:
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


# ------------------------------------------------------------------ 7. call order and coexistence
def test_call_order_and_a_world_beside_the_ensemble(nb, orc):
    C = nb._capi
    h = C.EnsembleHandle(0)
    try:
        assert h.shape == (0, 0)
        for call in (lambda: h.update(0.1, 1), lambda: h.update(0.1, 0), h.accel, h.download):
            with pytest.raises(C.NBodyError) as e:
                call()
            assert e.value.code == C.ERR_INVALID and "ensemble" in str(e.value)
        with pytest.raises(C.NBodyError) as e:
            h.upload(1, 4097, np.zeros((4097, 2), F32), np.zeros((4097, 2), F32), None)
        assert e.value.code == C.ERR_INVALID and "ensemble" in str(e.value) and h.shape == (0, 0)
    finally:
        h.close()

    pos, vel, w = _worlds(nb, 200, 3, seed=750, awkward_at=-1)
    cnt = nb.Counting()
    with nb.Ensemble(pos, vel, w, arith="auto") as ens:
        ens.update(0.1, cnt, n_steps=0)
        p, v, _ = ens.particles()
        assert p.tobytes() == pos.tobytes() and v.tobytes() == vel.tobytes() and cnt.sum_gravity == 0.0
        with pytest.raises(C.NBodyError):
            ens.update(0.1, None, n_steps=-1)
        ens.update(0.1, cnt, n_steps=2)
        assert cnt.sum_gravity > 0.0 and cnt.build_bvh == 0.0 and cnt.post_calculations == 0.0

    def world_steps(between=None):
        world = nb.World(G["ic_pos"], G["ic_vel"], G["ic_weight"], method="direct", arith="exact")
        try:
            for _ in range(3):
                world.update(0.1, None, n_steps=2)
                if between:
                    between()
            return world.particles()[:2]
        finally:
            world.close()

    alone = world_steps()
    with nb.Ensemble(pos, vel, w, arith="fast") as ens:
        beside = world_steps(lambda: ens.update(0.1, None, n_steps=1))
        pe, _, _ = ens.particles()
    assert alone[0].tobytes() == beside[0].tobytes() and alone[1].tobytes() == beside[1].tobytes()
    with nb.Ensemble(pos, vel, w, arith="fast") as ens:
        ens.update(0.1, None, n_steps=3)
        assert ens.particles()[0].tobytes() == pe.tobytes()
