"""Ragged restricted ensembles in f64 on the device (nb.RaggedRestrictedEnsemble64 over nbody_rr64_*): double-precision worlds of
different sizes, each with a tracer count of its own, stepped together.  Every world is compared on its own — EXACT and AUTO (the
exact chain in f64) with the oracle's update_direct (bodies) and direct_accel at the tracers + Euler on float64, bit for bit; FAST
with nb.RestrictedEnsemble64 holding that world alone and with nb.RaggedEnsemble64 holding the same worlds, bit for bit (the
kernels share their block bodies), and with the frozen f64 contract of DESIGN §5 (1e-12 of sum |term|).  Needs an MI355X.

Sizes: n on either side of every launch class boundary that the tracers' plan has (128 / 129, 256 / 257), 1, 2 and 7 (the bodies
split their sources over lanes, the tracers never do; none is a multiple of the term block of 8), 3272 / 3273 on either side of
the 64 KiB dynamic-LDS limit (65 440 / 65 600 B), which the tracers' kernel has to have raised for itself, 4096 (81 920 B); m on
either side of a lane row (256), of a tile (512) and of two tiles, one tracer, and none."""
import numpy as np
import pytest

import test_gpu_ragged64 as RG
from _tol import fast_error
from test_gpu_ensemble64 import FAST_RTOL, _fast_worlds
from test_gpu_ragged64 import _assert_worlds_equal, _same_bits
from test_gpu_restricted64 import _exact_accel, _exact_steps, _tracers_for
from test_gpu_tracers import _outside_fast

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
DT = 0.1
CLAMP = 0.001

N11 = [257, 1, 4096, 7, 129, 2, 1000, 65, 128, 3273, 3272]
M11 = [256, 1, 300, 257, 513, 0, 1025, 600, 512, 300, 2]


def _tracers_of(pos, counts, seed, with_skip=True):
    """One entry per world: None where the count is 0, else test_gpu_restricted64._tracers_for of that world alone."""
    out = []
    for k, m in enumerate(counts):
        if not m:
            out.append(None)
            continue
        tp, tv = _tracers_for(pos[k][None], m, seed + 31 * k, with_skip=with_skip)
        out.append((tp[0], tv[0]))
    return out


def _oracle_world(orc, p, v, w, tr, steps, clamp=CLAMP):
    """One world alone through the oracle -> (pos, vel, tracer pos, tracer vel); the last two None without tracers."""
    if tr is None or not len(tr[0]):
        rp, rv = RG._oracle_steps(orc, [p], [v], [w], steps, clamp=clamp, delta=DT)
        return rp[0], rv[0], None, None
    rp, rv, rtp, rtv = _exact_steps(orc, p[None], v[None], w[None], tr[0][None], tr[1][None], steps, clamp=clamp)
    return rp[0], rv[0], rtp[0], rtv[0]


def _assert_equals_the_oracle(orc, pos, vel, w, tracers, got, steps, what, clamp=CLAMP):
    p, v, tr = got
    for k in range(len(pos)):
        rp, rv, rtp, rtv = _oracle_world(orc, pos[k], vel[k], w[k], tracers[k], steps, clamp=clamp)
        assert _same_bits(p[k], rp) and _same_bits(v[k], rv), f"{what}: bodies of world {k} (n = {len(pos[k])})"
        if rtp is None:
            assert tr[k][0].shape == tr[k][1].shape == (0, 2), k
        else:
            assert _same_bits(tr[k][0], rtp) and _same_bits(tr[k][1], rtv), f"{what}: tracers of world {k} (n = {len(pos[k])}, m = {len(rtp)})"


def _run(nb, pos, vel, w, tracers, arith, calls=(3,), **kw):
    with nb.RaggedRestrictedEnsemble64(pos, vel, w, tracers, arith=arith, **kw) as r:
        for k in calls:
            r.update(DT, None, n_steps=k)
        p, v, _ = r.particles()
        return p, v, r.tracers()


def _restricted_alone(nb, p, v, w, tr, arith, steps):
    """nb.RestrictedEnsemble64 holding this one world -> (pos, vel, tracer pos, tracer vel, tracer accel at the start)."""
    tracers = None if tr is None else (tr[0][None], tr[1][None])
    with nb.RestrictedEnsemble64(p[None], v[None], w[None], tracers, arith=arith) as r:
        ta = r.tracers_accel()
        r.update(DT, None, n_steps=steps)
        pp, vv, _ = r.particles()
        gp, gv = r.tracers()
        return pp[0], vv[0], gp[0], gv[0], ta[0]


def _assert_tracers_equal(got, want, what):
    assert len(got) == len(want), what
    for k in range(len(want)):
        assert _same_bits(got[k][0], want[k][0]) and _same_bits(got[k][1], want[k][1]), f"{what}: tracers of world {k}"


@pytest.fixture(scope="module")
def eleven(nb):
    """The eleven worlds of tests 1 and 3, in scrambled size order; world 4 (n = 129) is the awkward one (an inf, a NaN, -0,
    subnormal differences: under FAST it routes to EXACT and its neighbours do not)."""
    pos, vel, w = RG._worlds(nb, N11, seed=5100, awkward_at=(4,))
    return pos, vel, w, _tracers_of(pos, M11, 5200)


# ------------------------------------------------------------------ 1. EXACT against the oracle
def test_exact_every_world_equals_the_oracle_bit_for_bit(nb, orc, eleven):
    pos, vel, w, tracers = eleven
    with nb.RaggedRestrictedEnsemble64(pos, vel, w, tracers, arith="exact") as r:
        assert r.sizes == (N11, M11) and r.h.shape == (11, sum(N11)) and r.h.n_tracer_rows == sum(M11)
        assert [a.tolist() for a in r.h.sizes] == [N11, M11]
        r.update(DT, None, n_steps=3)
        p, v, w2 = r.particles()
        tr = r.tracers()
    assert [a.shape for a in p] == [(n, 2) for n in N11] and [t[0].shape for t in tr] == [(m, 2) for m in M11]
    assert all(a.dtype == F64 for a in p + v) and all(t[0].dtype == t[1].dtype == F64 for t in tr)
    assert all(np.array_equal(a, b) for a, b in zip(w2, w))
    _assert_equals_the_oracle(orc, pos, vel, w, tracers, (p, v, tr), 3, "EXACT")
    assert not np.array_equal(tr[0][0], tracers[0][0])          # (and the tracers moved)


# ------------------------------------------------------------------ 2. the launch above 64 KB of LDS, on its own
def test_the_large_lds_launch(nb, orc):
    """The only test whose tracers' launch needs rr64_tracers' own raised limit: a class whose largest world with tracers has
    n >= 3273.  Without the raise the launch is refused and update() raises."""
    ns, ms = [4096, 3273, 7], [300, 513, 1]
    pos, vel, w = RG._worlds(nb, ns, seed=5300)
    tracers = _tracers_of(pos, ms, 5400)
    plan = nb.rr_plan(ns, ms, dtype=F64)
    assert plan["lds_bytes"].tolist() == [160, 81920] and plan["blocks"].tolist() == [1, 3]
    got = _run(nb, pos, vel, w, tracers, "exact", calls=(1,))
    _assert_equals_the_oracle(orc, pos, vel, w, tracers, got, 1, "large LDS, EXACT")
    fast = _run(nb, pos, vel, w, tracers, "fast", calls=(1,))
    for k in range(3):
        up, uv, utp, utv, _ = _restricted_alone(nb, pos[k], vel[k], w[k], tracers[k], "fast", 1)
        assert _same_bits(fast[0][k], up) and _same_bits(fast[1][k], uv), k
        assert _same_bits(fast[2][k][0], utp) and _same_bits(fast[2][k][1], utv), k
    acc = {}
    for arith in ("exact", "fast"):
        with nb.RaggedRestrictedEnsemble64(pos, vel, w, tracers, arith=arith) as r:
            acc[arith] = r.tracers_accel()
    assert not _same_bits(acc["fast"][0], acc["exact"][0]) and not _same_bits(acc["fast"][1], acc["exact"][1])   # (FAST ran)
    # the tracers of the 4096-body world removed: the class's LDS drops to that of 3273, still above 64 KB
    cut, mc = [None, tracers[1], tracers[2]], [0, 513, 1]
    plan = nb.rr_plan(ns, mc, dtype=F64)
    assert plan["lds_bytes"].tolist() == [160, 65600] and plan["blocks"].tolist() == [1, 2] and plan["lds_bytes"][1] > 65536
    for arith, full in (("exact", got), ("fast", fast)):
        p, v, tr = _run(nb, pos, vel, w, cut, arith, calls=(1,))
        assert tr[0][0].shape == (0, 2)
        for k in (1, 2):
            assert _same_bits(tr[k][0], full[2][k][0]) and _same_bits(tr[k][1], full[2][k][1]), (arith, k)
        _assert_worlds_equal(p, full[0], f"{arith} positions")


# ------------------------------------------------------------------ 3. FAST and AUTO = the uniform handles, bit for bit
@pytest.mark.parametrize("arith", ["fast", "auto"])
def test_every_world_equals_the_uniform_handles_bit_for_bit(nb, eleven, arith):
    pos, vel, w, tracers = eleven
    p, v, tr = _run(nb, pos, vel, w, tracers, arith)
    for k, (n, m) in enumerate(zip(N11, M11)):
        up, uv, utp, utv, _ = _restricted_alone(nb, pos[k], vel[k], w[k], tracers[k], arith, 3)
        assert _same_bits(p[k], up) and _same_bits(v[k], uv), f"n = {n}: bodies differ from nb.RestrictedEnsemble64 of that world alone"
        assert utp.shape == (m, 2) and _same_bits(tr[k][0], utp) and _same_bits(tr[k][1], utv), \
            f"n = {n}, m = {m}: tracers differ from nb.RestrictedEnsemble64 of that world alone"
        assert not m or not np.array_equal(tr[k][0], tracers[k][0]), k
    with nb.RaggedEnsemble64(pos, vel, w, arith=arith) as rag:
        rag.update(DT, None, n_steps=3)
        rp, rv, _ = rag.particles()
    _assert_worlds_equal(p, rp, "positions against nb.RaggedEnsemble64")
    _assert_worlds_equal(v, rv, "velocities against nb.RaggedEnsemble64")


# ------------------------------------------------------------------ 4. tile edges
def test_tile_edges(nb, orc):
    """Every m around a multiple of a lane row and of a tile, in worlds of 7 bodies with one world of 300 between them: EXACT
    against the oracle, and FAST against itself with every m halved (the first half of the tracers alone: other tiles, other
    lanes, other rows of the table, the same bits)."""
    ms = [1, 255, 256, 257, 511, 700, 512, 513, 1023, 1025, 2049]
    ns = [7] * 5 + [300] + [7] * 5
    pos, vel, w = RG._worlds(nb, ns, seed=5500)
    tracers = _tracers_of(pos, ms, 5600)
    got = _run(nb, pos, vel, w, tracers, "exact", calls=(1,))
    _assert_equals_the_oracle(orc, pos, vel, w, tracers, got, 1, "tile edges")
    hs = [max(1, m // 2) for m in ms]
    with nb.RaggedRestrictedEnsemble64(pos, vel, w, tracers, arith="fast") as r:
        full = r.tracers_accel()
        r.set_tracers([(t[0][:h], t[1][:h]) for t, h in zip(tracers, hs)])
        assert r.sizes == (ns, hs)
        half = r.tracers_accel()
    for k, (m, h) in enumerate(zip(ms, hs)):
        assert full[k].shape == (m, 2) and half[k].shape == (h, 2) and full[k].dtype == F64
        assert _same_bits(full[k][:h], half[k]), (k, m)
        inside = ~_outside_fast(tracers[k][0])
        assert np.all(np.isfinite(full[k][inside])) and np.any(full[k][inside] != 0), (k, m)


# ------------------------------------------------------------------ 5. FAST within the frozen f64 contract
def test_fast_tracers_within_1e12(nb, orc):
    """|a - a_ref|_1 <= 1e-12 * sum_j |term_j|_1 per tracer against direct_accel(accum="f64"): DESIGN §5, the yardstick and the
    helper of test_gpu_restricted64.py."""
    galaxy = nb.scenes.galaxy(dtype=F64)
    per_n = [_fast_worlds(nb, galaxy, n) for n in (2, 64, 1000, 4096)]     # each (pos[3,n,2], vel[3,n,2], w[3,n])
    pos, vel, w = ([np.ascontiguousarray(per_n[i][x][j]) for j in range(3) for i in range(4)] for x in range(3))
    assert [len(p) for p in pos] == [2, 64, 1000, 4096] * 3               # interleaved: 2, 64, 1000, 4096, 2, ...
    counts = [600, 300, 513, 257] * 3
    tracers = _tracers_of(pos, counts, 5700, with_skip=False)             # all finite: on, near and away from bodies
    with nb.RaggedRestrictedEnsemble64(pos, vel, w, tracers, arith="fast") as r:
        acc = r.tracers_accel()
    assert FAST_RTOL == 1e-12
    ran_fast = False
    for k in range(12):
        tp = tracers[k][0]
        assert np.all(np.isfinite(tp)) and acc[k].dtype == F64 and acc[k].shape == (counts[k], 2)
        ref, norm = orc.direct_accel(pos[k], w[k], target_pos=tp, accum="f64", nthreads=16)
        native, _ = orc.direct_accel(pos[k], w[k], target_pos=tp, accum="native", nthreads=16)
        assert np.all(np.isfinite(acc[k])), k
        r = float(fast_error(acc[k], ref, norm).max())
        print(f"[tol] f64 ragged restricted FAST n={len(pos[k])} world {k}: max {r:.2e}")
        assert r <= FAST_RTOL, (len(pos[k]), k, r)
        ran_fast |= not _same_bits(acc[k], native)
    assert ran_fast


# ------------------------------------------------------------------ 6. a tracer on a body sees what the body sees
def test_fast_a_tracer_on_a_body_gets_the_bodys_bits(nb):
    ns = [129, 300, 4096]
    pos, vel, w = RG._worlds(nb, ns, seed=5800)
    assert all(np.all(np.isfinite(p)) for p in pos)
    tracers = [(p.copy(), v.copy()) for p, v in zip(pos, vel)]
    with nb.RaggedRestrictedEnsemble64(pos, vel, w, tracers, arith="fast") as r:
        body, tracer = r.accel(), r.tracers_accel()
    for k, n in enumerate(ns):
        assert body[k].shape == tracer[k].shape == (n, 2) and body[k].tobytes() == tracer[k].tobytes(), n
        assert np.any(body[k] != 0)


# ------------------------------------------------------------------ 7. independence
@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_a_tracer_depends_on_its_own_state_and_its_worlds_bodies_alone(nb, arith):
    ns, ms = [300, 7, 129, 300, 64, 1000], [600, 5, 0, 700, 513, 40]
    pos, vel, w = RG._worlds(nb, ns, seed=5900, awkward_at=(0,))   # (under FAST world 0 routes to EXACT, its neighbours do not)
    tracers = _tracers_of(pos, ms, 6000)                           # (the skip cases at the end: FAST's per-tracer exception)
    k = 3
    p0, v0, tr0 = _run(nb, pos, vel, w, tracers, arith)
    assert not np.array_equal(tr0[k][0], tracers[k][0])
    # the other worlds replaced by worlds of other sizes and contents, another launch class among them, and reordered: the world
    # is now second of three, its body rows and its tracer rows start elsewhere, and the table around its items is another
    op, ov, ow = RG._worlds(nb, [4096, 2], seed=5950)
    otr = _tracers_of(op, [100, 1], 6050)
    p, v, tr = _run(nb, [op[0], pos[k], op[1]], [ov[0], vel[k], ov[1]], [ow[0], w[k], ow[1]], [otr[0], tracers[k], otr[1]], arith)
    assert _same_bits(tr[1][0], tr0[k][0]) and _same_bits(tr[1][1], tr0[k][1])
    assert _same_bits(p[1], p0[k]) and _same_bits(v[1], v0[k])
    # the same worlds in reverse order
    p, v, tr = _run(nb, pos[::-1], vel[::-1], w[::-1], tracers[::-1], arith)
    _assert_worlds_equal(p[::-1], p0, "reversed: positions")
    _assert_worlds_equal(v[::-1], v0, "reversed: velocities")
    _assert_tracers_equal(tr[::-1], tr0, "reversed")
    # one world's bodies changed (world 4: another seed): every other world keeps its bits, world 4's tracers do not
    cp, cv, cw = RG._worlds(nb, [ns[4]], seed=5990)
    p, v, tr = _run(nb, pos[:4] + cp + pos[5:], vel[:4] + cv + vel[5:], w[:4] + cw + w[5:], tracers, arith)
    for j in range(len(ns)):
        same = _same_bits(tr[j][0], tr0[j][0]) and _same_bits(tr[j][1], tr0[j][1])
        assert same == (j != 4), j
        assert j == 4 or (_same_bits(p[j], p0[j]) and _same_bits(v[j], v0[j])), j
    # its own m cut: 700 -> 100 (two tiles -> one, every later tracer row moves), and to one tracer from the second tile
    cut = list(tracers)
    cut[k] = (tracers[k][0][:100], tracers[k][1][:100])
    p, v, tr = _run(nb, pos, vel, w, cut, arith)
    assert _same_bits(tr[k][0], tr0[k][0][:100]) and _same_bits(tr[k][1], tr0[k][1][:100])
    cut[k] = (tracers[k][0][600:601], tracers[k][1][600:601])
    p, v, tr = _run(nb, pos, vel, w, cut, arith)
    assert _same_bits(tr[k][0], tr0[k][0][600:601]) and _same_bits(tr[k][1], tr0[k][1][600:601])
    for j in range(len(ns)):
        assert _same_bits(p[j], p0[j]), j                          # (and no body noticed)
        assert j == k or (_same_bits(tr[j][0], tr0[j][0]) and _same_bits(tr[j][1], tr0[j][1])), j


# ------------------------------------------------------------------ 8. routing under "fast"
def test_fast_a_nan_body_makes_its_world_exact_and_no_other(nb, orc):
    ns, ms = [200, 150, 200, 1000], [600, 700, 300, 513]           # worlds 0 and 2 share world 1's launch, world 3 does not
    pos, vel, w = RG._worlds(nb, ns, seed=6100)
    tracers = _tracers_of(pos, ms, 6200, with_skip=False)          # (made from the clean bodies: all finite)
    pos[1][7] = (np.nan, 3.0)
    p, v, tr = _run(nb, pos, vel, w, tracers, "fast", calls=(2,))
    rp, rv, rtp, rtv = _oracle_world(orc, pos[1], vel[1], w[1], tracers[1], 2)
    assert _same_bits(p[1], rp) and _same_bits(v[1], rv)
    assert _same_bits(tr[1][0], rtp) and _same_bits(tr[1][1], rtv)
    # the routes themselves, in the accelerations at the initial state: world 1 EXACT, the others FAST — the bits of
    # nb.RestrictedEnsemble64 holding that world alone, and not the exact chain's
    with nb.RaggedRestrictedEnsemble64(pos, vel, w, tracers, arith="fast") as r:
        acc = r.tracers_accel()
    for k in range(len(ns)):
        ex = _exact_accel(orc, pos[k][None], w[k][None], tracers[k][0][None])[0]
        assert _same_bits(acc[k], ex) == (k == 1), k
        up, uv, utp, utv, uta = _restricted_alone(nb, pos[k], vel[k], w[k], tracers[k], "fast", 2)
        assert _same_bits(acc[k], uta), k
        assert _same_bits(p[k], up) and _same_bits(v[k], uv) and _same_bits(tr[k][0], utp) and _same_bits(tr[k][1], utv), k


def test_fast_a_tracer_outside_the_domain_takes_its_exact_value(nb, orc):
    ns, ms = [200, 65, 300], [700, 300, 1025]
    pos, vel, w = RG._worlds(nb, ns, seed=6300)
    tracers = _tracers_of(pos, ms, 6400, with_skip=False)
    plain = [(t[0].copy(), t[1]) for t in tracers]
    odd = [np.zeros(m, bool) for m in ms]
    for k, i, at in ((0, 300, (2.0 ** 101, 3.0)), (2, 511, (50000.0, 1e-305)), (2, 512, (np.inf, 1.0)), (2, 1024, (1e-310, 50000.0))):
        tracers[k][0][i] = at
        odd[k][i] = True
    assert all(np.array_equal(_outside_fast(tracers[k][0]), odd[k]) for k in range(3))
    with nb.RaggedRestrictedEnsemble64(pos, vel, w, tracers, arith="fast") as r:
        mixed = r.tracers_accel()
        r.set_tracers(plain)
        fast = r.tracers_accel()
    for k in range(len(ns)):
        ex = _exact_accel(orc, pos[k][None], w[k][None], tracers[k][0][None])[0]
        assert _same_bits(mixed[k][odd[k]], ex[odd[k]]), k
        assert mixed[k][~odd[k]].tobytes() == fast[k][~odd[k]].tobytes(), k      # the neighbours keep the bits they have without them
        assert not _same_bits(mixed[k][~odd[k]], ex[~odd[k]]), k                 # ... FAST bits
    # a clamp of 0: everything EXACT
    got = _run(nb, pos, vel, w, tracers, "fast", calls=(2,), clamp=0.0)
    _assert_equals_the_oracle(orc, pos, vel, w, tracers, got, 2, "clamp 0", clamp=0.0)


# ------------------------------------------------------------------ 9. degenerate shapes
@pytest.mark.parametrize("arith", ["fast", "exact"])
def test_degenerate_shapes_are_the_handles_they_degenerate_to(nb, arith):
    ns = [300, 7, 129, 64]
    pos, vel, w = RG._worlds(nb, ns, seed=6500, awkward_at=(2,))
    # no tracers at all: a RaggedEnsemble64 under another name
    with nb.RaggedEnsemble64(pos, vel, w, arith=arith) as rag:
        rag.update(DT, None, n_steps=3)
        rp, rv, _ = rag.particles()
        ra = rag.accel()
    for tracers in (None, [None] * 4, [(np.zeros((0, 2), F64), np.zeros((0, 2), F64))] * 4):
        with nb.RaggedRestrictedEnsemble64(pos, vel, w, tracers, arith=arith) as r:
            assert r.sizes == (ns, [0] * 4) and r.h.n_tracer_rows == 0
            r.update(DT, None, n_steps=3)
            p, v, _ = r.particles()
            a = r.accel()
            tr, ta = r.tracers(), r.tracers_accel()
        _assert_worlds_equal(p, rp, "positions")
        _assert_worlds_equal(v, rv, "velocities")
        _assert_worlds_equal(a, ra, "accelerations")
        assert [t[0].shape for t in tr] == [(0, 2)] * 4 and [t.shape for t in ta] == [(0, 2)] * 4
    # equal n and equal m: a RestrictedEnsemble64 under another name; and one world
    n, m = 300, 600
    for b in (3, 1):
        pos, vel, w = RG._worlds(nb, [n] * b, seed=6600, awkward_at=(1,))
        tracers = _tracers_of(pos, [m] * b, 6700)
        stacked = (np.stack([t[0] for t in tracers]), np.stack([t[1] for t in tracers]))
        with nb.RestrictedEnsemble64(np.stack(pos), np.stack(vel), np.stack(w), stacked, arith=arith) as u:
            u.update(DT, None, n_steps=3)
            up, uv, _ = u.particles()
            utp, utv = u.tracers()
            uta = u.tracers_accel()
        with nb.RaggedRestrictedEnsemble64(pos, vel, w, tracers, arith=arith) as r:
            r.update(DT, None, n_steps=3)
            p, v, _ = r.particles()
            tr, ta = r.tracers(), r.tracers_accel()
            _assert_worlds_equal(p, list(up), "positions")
            _assert_worlds_equal(v, list(uv), "velocities")
            _assert_worlds_equal([t[0] for t in tr], list(utp), "tracer positions")
            _assert_worlds_equal([t[1] for t in tr], list(utv), "tracer velocities")
            _assert_worlds_equal(ta, list(uta), "tracer accelerations")
            # set_tracers(None) removes the tracers; the downloads then return empties with NBODY_OK
            r.set_tracers(None)
            assert r.sizes == ([n] * b, [0] * b) and r.h.n_tracer_rows == 0
            assert [t[0].shape for t in r.tracers()] == [(0, 2)] * b and [t.shape for t in r.tracers_accel()] == [(0, 2)] * b
            gp, gv = r.h.download_tracers()
            assert gp.shape == gv.shape == (0, 2) and gp.dtype == F64 and r.h.tracers_accel().shape == (0, 2)
            p2, v2, _ = r.particles()                              # the bodies are where they were
            assert all(x.tobytes() == y.tobytes() for x, y in zip(p2 + v2, p + v))


# ------------------------------------------------------------------ 10. lifetime and errors
@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_steps_split_over_calls_and_download_order(nb, arith):
    ns, ms = [300, 7, 129, 3273], [600, 5, 0, 513]
    pos, vel, w = RG._worlds(nb, ns, seed=6800, awkward_at=(2,))
    tracers = _tracers_of(pos, ms, 6900)
    p0, v0, tr0 = _run(nb, pos, vel, w, tracers, arith)                    # 3 steps in one call; the bodies first
    with nb.RaggedRestrictedEnsemble64(pos, vel, w, tracers, arith=arith) as r:
        r.update(DT, None, n_steps=1)
        r.update(DT, None, n_steps=2)
        tr = r.tracers()                                                   # the tracers first, twice, then the bodies
        again = r.tracers()
        p, v, _ = r.particles()
    _assert_worlds_equal(p, p0, "1 + 2 steps: positions")
    _assert_worlds_equal(v, v0, "1 + 2 steps: velocities")
    _assert_tracers_equal(tr, tr0, "1 + 2 steps")
    _assert_tracers_equal(again, tr0, "a second download")


def test_call_order_and_booking(nb):
    C = nb._capi
    tp = np.zeros((4, 2), F64)
    h = C.RR64Handle(0)
    try:
        assert h.shape == (0, 0) and h.n_tracer_rows == 0 and [a.tolist() for a in h.sizes] == [[], []]
        for call in (lambda: h.update(DT, 1), lambda: h.update(DT, 0), h.accel, h.download, h.tracers_accel, h.download_tracers,
                     lambda: h.upload_tracers([4], tp, tp)):
            with pytest.raises(C.NBodyError) as e:
                call()
            assert e.value.code == C.ERR_INVALID and "ragged restricted" in str(e.value)
        for bad in ([4, 4097], [0, 4], []):
            n = max(sum(bad), 1)
            with pytest.raises(C.NBodyError) as e:
                h.upload(np.array(bad, np.int64), np.zeros((n, 2), F64), np.zeros((n, 2), F64), None)
            assert e.value.code == C.ERR_INVALID and "ragged restricted" in str(e.value) and h.shape == (0, 0)
    finally:
        h.close()
    ns, ms = [200, 9, 600], [300, 0, 513]
    pos, vel, w = RG._worlds(nb, ns, seed=7000)
    tracers = _tracers_of(pos, ms, 7100, with_skip=False)
    cnt = nb.Counting()
    with nb.RaggedRestrictedEnsemble64(pos, vel, None, tracers) as r:     # no weights: all 1; booking: the whole call under sum_gravity
        assert r.h.get_params().arith == C.ARITH_AUTO                     # (the constructor's default; in f64 the exact chain)
        r.update(DT, cnt, n_steps=0)
        p, v, w1 = r.particles()
        tr = r.tracers()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(p + v, pos + vel)) and cnt.sum_gravity == 0.0
        assert all(t is None or (g[0].tobytes() == t[0].tobytes() and g[1].tobytes() == t[1].tobytes()) for g, t in zip(tr, tracers))
        assert all(a.dtype == np.uint32 and (a == 1).all() for a in w1)
        with pytest.raises(C.NBodyError):
            r.update(DT, None, n_steps=-1)
        r.update(DT, cnt, n_steps=2)
        assert cnt.sum_gravity > 0.0 and cnt.build_bvh == 0.0 and cnt.post_calculations == 0.0


def test_a_refused_upload_leaves_state_as_it_was_and_a_second_upload_replaces_it(nb, orc):
    """An upload refused for its arguments changes nothing.  The C calls on the handle itself: the Python class would refuse first."""
    C = nb._capi
    ns, ms = [3, 130, 65], [5, 0, 600]
    pos, vel, w = RG._worlds(nb, ns, seed=7200)
    tracers = _tracers_of(pos, ms, 7300, with_skip=False)
    rows, trows = sum(ns), sum(ms)
    z = np.zeros((trows, 2), F64)
    big = np.zeros((4097 + 3, 2), F64)
    with nb.RaggedRestrictedEnsemble64(pos, vel, w, tracers, arith="exact") as r:
        r.update(DT, None, n_steps=1)
        before = (*r.h.download(), *r.h.download_tracers(), r.h.accel(), r.h.tracers_accel())
        assert before[0].shape == (rows, 2) and before[2].shape == (trows, 2) and before[2].dtype == F64
        assert not np.array_equal(before[0], np.concatenate(pos)) and not np.array_equal(before[2][:5], tracers[0][0])
        refused = (lambda: r.h.upload(np.array([3, 4097], np.int64), big, big, None),          # a size outside the limits
                   lambda: r.h.upload(np.array([3, 0], np.int64), big, big, None),
                   lambda: r.h.upload(np.array(ns, np.int64), None, np.concatenate(vel), None),   # a NULL array
                   lambda: r.h.upload_tracers([5, 0], z, z),                                    # not the bodies' n_worlds
                   lambda: r.h.upload_tracers([5, -1, 600], z, z),                              # a negative count
                   lambda: r.h.upload_tracers([5, 0, 1 << 26], z, z),                           # more than 2^26 in all
                   lambda: r.h.upload_tracers(ms, None, z), lambda: r.h.upload_tracers(ms, z, None))
        for call in refused:
            with pytest.raises(C.NBodyError) as e:
                call()
            assert e.value.code == C.ERR_INVALID and "ragged restricted" in str(e.value)
            assert r.h.shape == (3, rows) and r.h.n_tracer_rows == trows and [a.tolist() for a in r.h.sizes] == [ns, ms]
        after = (*r.h.download(), *r.h.download_tracers(), r.h.accel(), r.h.tracers_accel())
        for x, y in zip(after, before):
            assert x.shape == y.shape and x.tobytes() == y.tobytes()
        r.update(DT, None, n_steps=1)
        p, v, _ = r.particles()
        _assert_equals_the_oracle(orc, pos, vel, w, tracers, (p, v, r.tracers()), 2, "after the refusals")
        r.h.upload_tracers([0, 0, 0], None, None)                   # all zero needs no arrays
        assert r.h.n_tracer_rows == 0 and r.h.shape == (3, rows)
        # a second upload, of other sizes and counts: more worlds, other launches; the tracers of the first go with its bodies
        ns2, ms2 = [65, 1025, 2, 300], [513, 7, 0, 1]
        pos2, vel2, w2 = RG._worlds(nb, ns2, seed=7250, awkward_at=(0,))
        tracers2 = _tracers_of(pos2, ms2, 7350)
        r.set_tracers(tracers)
        r.upload(pos2, vel2, w2)
        assert r.sizes == (ns2, [0] * 4) and r.h.n_tracer_rows == 0
        r.set_tracers(tracers2)
        assert r.sizes == (ns2, ms2) and r.h.shape == (4, sum(ns2)) and r.h.n_tracer_rows == sum(ms2)
        r.update(DT, None, n_steps=3)
        p, v, w3 = r.particles()
        _assert_equals_the_oracle(orc, pos2, vel2, w2, tracers2, (p, v, r.tracers()), 3, "second upload")
        assert all(np.array_equal(a, b) for a, b in zip(w3, w2))
