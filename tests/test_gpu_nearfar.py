"""The near/far split of the direct step (csrc/nearfar.hip) and its consumers at their edges.  Needs an MI355X.

Through the door (nbody_selftest_nearfar: the split and nothing else) the classifier's near SET, near list, scan, flag words, far
copy and inverse masses are compared with the numpy restatement of tests/_nearfar.py, exactly: bytes for the floats.  Fingerprint
merges of super-cells can only ADD near bodies, deterministically: the device set must always contain the restated one, and for
the committed seeds it equals it (no seed had to be changed for a merge).
Through whole steps (NBODY_DIRECT_NEARFAR=2) every consumer of the near list is compared with the oracle's exactly accumulated
sum on EVERY target under the frozen FAST tolerance, after a CPU-side proof that one planted pair summed without the clamp would
break that tolerance by orders of magnitude."""
import numpy as np
import pytest

from tests import _nearfar as NF
from tests._tol import ACC_RTOL, check_fast, fast_error

pytestmark = pytest.mark.gpu
F32 = np.float32
N = NF.N_SCENE


# ---------------------------------------------------------------------------------------------------- through the door
def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _check_door(C, pos, mass=None, heavy_base=0.0, use_hazard=True, couples=True, with_minv=False):
    """Everything the door hands out against the restatement; returns (result, restated near set)."""
    r = C.selftest_nearfar(pos, mass, heavy_base=heavy_base, use_hazard=use_hazard, couples=couples, with_minv=with_minv)
    want = NF.near(pos, mass, heavy_base)
    assert np.all(r["is_near"] <= 1)
    dev = r["is_near"] != 0
    print(f"near bodies: restated {want.sum()}, device {dev.sum()}")
    assert np.all(dev[want]), "a body with a neighbour within its 3 x 3 cells was classified far"
    assert np.array_equal(dev, want)          # (an extra near body here would be a fingerprint merge: see the module's docstring)
    assert np.array_equal(r["near_list"], np.flatnonzero(want))
    assert np.array_equal(r["scan"], np.cumsum(want) - want)
    assert r["flags"] == NF.expected_flags(pos, want, use_hazard)
    assert np.array_equal(_bits(r["far"]), _bits(NF.expected_far(pos, want, couples)))
    if with_minv:
        assert np.array_equal(_bits(r["minv"][:len(pos)]), _bits(NF.expected_minv(mass)))
    return r, want


@pytest.fixture(scope="module")
def scene():
    pos, rows = NF.planted_scene()
    return pos, rows, NF.near(pos)


@pytest.mark.parametrize("couples", [True, False])
def test_planted_scene_through_the_door(nb, scene, couples):
    pos, _, near = scene
    mass = (np.arange(N) % 7 + 1).astype(F32)
    mass[[5, 4000, N - 2]] = 0.0, F32(2 ** 32 - 1), 0.0
    r, want = _check_door(nb._capi, pos, mass, couples=couples, with_minv=couples)
    assert r["flags"] == (0, 0, 336, 0) and np.array_equal(want, near)
    r0, _ = _check_door(nb._capi, pos, None, couples=couples)          # no masses at all: the same split
    assert np.array_equal(_bits(r0["far"]), _bits(r["far"]))


def test_heavy_base_adds_the_odd_masses_and_nothing_else(nb, scene):
    pos, _, near = scene
    odd = [0, 1, N - 1]
    assert not near[odd].any()          # (lattice singles under this seed: they join the near set by their masses alone)
    mass = np.full(N, 3, F32)
    mass[odd] = 75e6, 1.0, 4e9
    r, want = _check_door(nb._capi, pos, mass, heavy_base=3.0)
    assert r["flags"] == (0, 0, 339, 0) and np.array_equal(np.flatnonzero(want & ~near), odd)


@pytest.mark.parametrize("n_near,state", [(383, 0), (384, 0), (385, 1)])
def test_decision_rule_at_its_edge(nb, n_near, state):
    pos = NF.counted_scene(n_near)
    r, _ = _check_door(nb._capi, pos)
    assert r["flags"] == (0, 0, n_near, state) and N // 64 == 384


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("sign", [1, -1])
def test_grid_range_edge(nb, scene, sign, axis):
    """One lattice single moved to the last f32 coordinate whose cell is in range (the split stands, the near set is right), then
    to the next f32 value, the first out of range (fallback flag, state 1)."""
    pos0, _, near = scene
    row = int(np.flatnonzero(~near)[100])
    inside, outside = NF.range_edge(sign)
    pos = pos0.copy()
    pos[row, axis] = inside
    r, want = _check_door(nb._capi, pos)
    assert r["flags"] == (0, 0, 336, 0) and np.array_equal(want, near)
    pos[row, axis] = outside
    r = nb._capi.selftest_nearfar(pos, use_hazard=True)
    want_flags = NF.expected_flags(pos, NF.near(pos), True)
    assert want_flags[:2] == (0, 1) and want_flags[3] == 1
    assert (r["flags"][0], r["flags"][1], r["flags"][3]) == (0, 1, 1)


N_PARTIAL = N + 37          # the last wave of nf_insert holds 37 bodies


@pytest.fixture(scope="module")
def scene_partial():
    return NF.planted_scene(n=N_PARTIAL, seed=3)[0]


@pytest.mark.parametrize("row", [0, 63, 64, N_PARTIAL - 1])
def test_fast_domain_edges_through_nf_insert(nb, scene_partial, row):
    """One value at FAST's domain edges in one coordinate of one body: the hazard flag and the state follow outside_fast() with
    use_hazard, and the hazard flag stays 0 without it.  (A coordinate of 2^60 also leaves the grid: the restatement says so.)"""
    C = nb._capi
    for axis in (0, 1):
        for v in NF.FAST_EDGE_VALUES:
            pos = scene_partial.copy()
            pos[row, axis] = v
            want_near = NF.near(pos)
            for use_hazard in (True, False):
                want = NF.expected_flags(pos, want_near, use_hazard)
                assert want[0] == int(use_hazard and bool(NF.outside_fast(v)))
                r = C.selftest_nearfar(pos, use_hazard=use_hazard)
                got = r["flags"]
                assert (got[0], got[1], got[3]) == (want[0], want[1], want[3]), (axis, float(v), use_hazard, got, want)
                if not want[1]:          # the grid holds every body: the near set is the restated one whatever the state
                    assert got == want and np.array_equal(r["is_near"] != 0, want_near), (axis, float(v), use_hazard)


@pytest.mark.parametrize("row", [0, 63, 64, 4096 + 37 - 1])
def test_fast_domain_edges_through_the_hazard_scan(nb, monkeypatch, row):
    """The same table through nbody_direct_step_dev at a size where the split is not chosen: direct_hazard_scan decides."""
    import torch
    C = nb._capi
    monkeypatch.delenv("NBODY_DIRECT_NEARFAR", raising=False)
    n = 4096 + 37
    pos0 = NF.lattice(n)
    dev = torch.device("cuda:0")
    tm = torch.ones(n, dtype=torch.float32, device=dev)
    acc = torch.empty((n, 2), dtype=torch.float32, device=dev)
    ws_bytes = C.direct_workspace_bytes(n, n)
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    for axis in (0, 1):
        for v in NF.FAST_EDGE_VALUES:
            pos = pos0.copy()
            pos[row, axis] = v
            tp = torch.from_numpy(pos).to(dev)
            C.direct_step_dev(stream, n, tp.data_ptr(), tm.data_ptr(), 0, n, None, None, acc.data_ptr(), 0.0, 0.001, C.ARITH_AUTO,
                              ws.data_ptr(), ws_bytes, uniform_mass=1.0)
            torch.cuda.synchronize()
            out = bool(NF.outside_fast(v))
            assert C.direct_workspace_peek(stream, ws.data_ptr()) == (int(out), 0, 0, 2 if out else 1), (axis, float(v))


# ---------------------------------------------------------------------------------------------------- through whole steps
@pytest.fixture
def force_nearfar(monkeypatch):
    monkeypatch.setenv("NBODY_DIRECT_NEARFAR", "2")


def _dev_accel(C, pos, w, uniform):
    """Every body's acceleration through nbody_direct_step_dev on a workspace of the test's own -> (acc, flag words)."""
    import torch
    n = len(pos)
    dev = torch.device("cuda:0")
    tp = torch.from_numpy(np.ascontiguousarray(pos, F32)).to(dev)
    tm = torch.from_numpy(w.astype(F32)).to(dev)
    acc = torch.empty((n, 2), dtype=torch.float32, device=dev)
    ws_bytes = C.direct_workspace_bytes(n, n)
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    C.direct_step_dev(stream, n, tp.data_ptr(), tm.data_ptr(), 0, n, None, None, acc.data_ptr(), 0.0, 0.001, C.ARITH_AUTO, ws.data_ptr(),
                      ws_bytes, uniform_mass=uniform)
    torch.cuda.synchronize()
    return acc.cpu().numpy(), C.direct_workspace_peek(stream, ws.data_ptr())


def _ctx_accel(ctx, C, pos, w):
    ctx.set_params(arith=C.ARITH_AUTO, clamp=0.001)
    ctx.upload(pos, np.zeros_like(pos), w)
    return ctx.accel_direct()


def _ref(orc, pos, w):
    return orc.direct_accel(pos, w, accum="f64", nthreads=16)


def _a_miss_would_show(orc, pos, w, rows, ref64, norm, label):
    """CPU only, before any GPU call: the reference once more with the clamp disabled for ONE planted adjacent-cell pair — what a
    step gives whose split calls both bodies far.  Both targets must then miss the tolerance; this is done for every planted
    adjacent-cell pair in turn and the smallest excess is printed (measured, error / ACC_RTOL: 5.2e5 equal masses, 6.0e4 free
    masses, 5.0e5 sparse, 4.7e5 three classes)."""
    worst = np.inf
    for a, b, _, d in rows:
        if max(abs(d[0]), abs(d[1])) != 1:
            continue
        for t, s in ((a, b), (b, a)):
            clamped = orc.pair(pos[t], pos[s], F32(w[s]), clamp=0.001).astype(np.float64)
            free = orc.pair(pos[t], pos[s], F32(w[s]), clamp=0.0).astype(np.float64)
            e = fast_error((ref64[t] - clamped + free)[None], ref64[t][None], norm[t:t + 1])[0]
            assert e > ACC_RTOL
            worst = min(worst, e / ACC_RTOL)
    print(f"[miss]{label} one pair without the clamp: error / ACC_RTOL >= {worst:.3g}")
    assert worst >= 100          # (a thinner margin asks for closer pairs: fractions 0.5 +- 0.45)
    return worst


@pytest.mark.parametrize("masses", ["equal", "free", "sparse"])
def test_planted_scene_through_the_streamed_consumers(nb, orc, force_nearfar, scene, masses):
    """direct_stream (equal masses), direct_stream_m (free masses) and the sparse route (one mass but for three bodies, which
    travel with the near list): state 0, the restated near count, every target within the frozen tolerance."""
    C = nb._capi
    pos, rows, near = scene
    if masses == "equal":
        w = np.ones(N, np.uint32)
    elif masses == "free":
        w = np.random.default_rng(11).integers(1, 1000, N).astype(np.uint32)
    else:
        w = np.full(N, 3, np.uint32)
        w[np.flatnonzero(~near)[[0, 700, -1]]] = 75_000_000, 750_000, 1
    hint = C.mass_hint(w)
    assert hint == {"equal": 1.0, "free": 0.0, "sparse": -3.0}[masses]
    n_near = int(NF.near(pos, w.astype(F32), heavy_base=max(-hint, 0.0)).sum())
    assert n_near == (339 if masses == "sparse" else 336)
    ref64, norm = _ref(orc, pos, w)
    _a_miss_would_show(orc, pos, w, rows, ref64, norm, f" {masses}")
    acc, flags = _dev_accel(C, pos, w, hint)
    assert flags == (0, 0, n_near, 0)
    check_fast(acc, ref64, norm, label=f" planted scene, {masses} masses")


def test_planted_scene_through_the_mass_classes(nb, orc, force_nearfar):
    """Three mass classes through a context at n = 32 768, the smallest size where classes engage (the far copy in class order)."""
    C = nb._capi
    n = 32768
    pos, rows = NF.planted_scene(n=n, seed=4)
    w = (np.arange(n) % 3 + 1).astype(np.uint32)
    assert C.mass_hint(w) == 0.0 and NF.near(pos).sum() == 336
    r = C.selftest_nearfar(pos)
    assert r["flags"] == (0, 0, 336, 0)          # the padded scene's split as the step will see it (the context's workspace is its own)
    ref64, norm = _ref(orc, pos, w)
    _a_miss_would_show(orc, pos, w, rows, ref64, norm, " classes")
    with C.Context(0) as ctx:
        acc = _ctx_accel(ctx, C, pos, w)
    check_fast(acc, ref64, norm, label=" planted scene, three mass classes")


def _mutual_accel(lab_ctx, C, monkeypatch, pos, w):
    monkeypatch.setenv("NBODY_DIRECT_NEARFAR", "2")
    monkeypatch.setenv("NBODY_DIRECT_MUTUAL_MIN_N", "0")
    monkeypatch.setenv("NBODY_DIRECT_ASM", "4")
    return _ctx_accel(lab_ctx, C, pos, w)


def test_planted_scene_through_the_mutual_pass(nb, orc, lab_ctx, monkeypatch, scene):
    C = nb._capi
    pos, rows, near = scene
    w = np.ones(N, np.uint32)
    ref64, norm = _ref(orc, pos, w)
    _a_miss_would_show(orc, pos, w, rows, ref64, norm, " mutual")
    assert C.selftest_nearfar(pos)["flags"] == (0, 0, 336, 0)
    acc = _mutual_accel(lab_ctx, C, monkeypatch, pos, w)
    check_fast(acc, ref64, norm, label=" planted scene, mutual pass")
    monkeypatch.setenv("NBODY_DIRECT_ASM", "3")          # ... and that was not direct_stream
    assert not np.array_equal(acc, _ctx_accel(lab_ctx, C, pos, w))


@pytest.mark.parametrize("n_near", [255, 256, 257, 384])
def test_direct_finish_lds_chunks(nb, orc, force_nearfar, n_near):
    """direct_finish takes the near sources 256 at a time through LDS: one short of a chunk, a whole chunk, one over, and the
    most the split allows at this size."""
    C = nb._capi
    pos = NF.counted_scene(n_near, seed=5)
    w = np.ones(N, np.uint32)
    acc, flags = _dev_accel(C, pos, w, 1.0)
    assert flags == (0, 0, n_near, 0)
    check_fast(acc, *_ref(orc, pos, w), label=f" direct_finish, {n_near} near sources")


@pytest.mark.parametrize("n_near", [0, 1, 63, 64, 65, 129])
def test_direct_mutual_near_rows(nb, orc, lab_ctx, monkeypatch, n_near):
    """direct_mutual_near takes 64 near bodies in flight: none, one (an odd mass: near by its mass alone), one short of a round,
    a whole round, one over, two rounds and one."""
    C = nb._capi
    w = np.ones(N, np.uint32)
    if n_near == 1:
        pos = NF.counted_scene(0, seed=6)
        w[12345] = 750_000
    else:
        pos = NF.counted_scene(n_near, seed=6)
    assert C.selftest_nearfar(pos, w.astype(F32), heavy_base=1.0)["flags"] == (0, 0, n_near, 0)
    acc = _mutual_accel(lab_ctx, C, monkeypatch, pos, w)
    check_fast(acc, *_ref(orc, pos, w), label=f" direct_mutual_near, {n_near} near bodies")
