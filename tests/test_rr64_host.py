"""Ragged restricted ensembles in f64 (nbody_rr64_*, nb.RaggedRestrictedEnsemble64, nb.rr_plan(dtype=float64)) without a GPU: the
declared names in both libraries, the refusal to run without a device, NULL-handle calls with an error slot of their own,
argument checks that must fire before any handle exists, and the tracers' launch plan under the f64 LDS function — pure host
code — checked block by block against a restatement."""
import ctypes
import os
import re

import numpy as np
import pytest

F32, F64 = np.float32, np.float64
NAMES = ["nbody_rr64_" + s for s in ("create", "destroy", "last_error", "set_params", "get_params", "upload", "download",
                                     "tracers_upload", "tracers_download", "num_worlds", "num_rows", "num_tracer_rows", "sizes",
                                     "update", "accel", "tracers_accel", "plan")]
PLAN_N = [1, 2, 7, 8, 9, 65, 128, 129, 256, 257, 512, 513, 1000, 1024, 1025, 2048, 2049, 3272, 3273, 4096]
PLAN_M = [0, 1, 511, 512, 513, 1023, 1024, 1025]
CAPS = (128, 256, 512, 1024, 2048, 4096)
TILE = 512


def _worlds(sizes, dtype=F64):
    return [np.zeros((n, 2), dtype) for n in sizes], [np.zeros((n, 2), dtype) for n in sizes]


def _tracers(counts, dtype=F64):
    return [None if m is None else (np.zeros((m, 2), dtype), np.zeros((m, 2), dtype)) for m in counts]


def _lds64(n):
    """A double2 position and a u32 weight per body, the rows padded to a multiple of the EXACT term block of 8."""
    return (n + 7) // 8 * 8 * 20


def _lds32(n):
    return (n + 1) // 2 * 24


def _class(n):
    return next(c for c, cap in enumerate(CAPS) if n <= cap)


# ------------------------------------------------------------------ names
def test_header_declares_the_rr64_calls_and_both_libraries_export_them(nb):
    C = nb._capi
    assert len(NAMES) == 17
    declared = C.declared_symbols()
    assert sorted(s for s in declared if s.startswith("nbody_rr64_")) == sorted(NAMES)
    assert sorted(s for s in C._SIGS if s.startswith("nbody_rr64_")) == sorted(NAMES)
    assert sorted(C._SIGS) == declared
    for path in (C.LIB_PATH, C.LAB_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in NAMES if not hasattr(lib, s)], path
    with open(C.HEADER_PATH) as f:
        head = f.read()
    assert int(re.search(r"#define\s+NBODY_ABI_VERSION\s+(\d+)", head).group(1)) == 3 == C.ABI_VERSION    # new symbols only
    assert "nbody_rr64" not in head                                         # declared in nbody_ensemble.h, which it includes
    with open(os.path.join(os.path.dirname(C.HEADER_PATH), "nbody_ensemble.h")) as f:
        ens = f.read()
    assert "typedef struct nbody_rr64 nbody_rr64;" in ens
    assert ens.index("typedef struct nbody_rr nbody_rr;") < ens.index("typedef struct nbody_rr64 nbody_rr64;")
    assert len(re.findall(r"#define\s+NBODY_RR_MAX_LAUNCHES\s+12\b", ens)) == 1 and C.RR_MAX_LAUNCHES == 12   # one constant for both
    # the prefix is its own: no call of this handle falls into the closed sets of the f32 sibling, the ragged or the restricted handles
    assert not [s for s in NAMES if s.startswith(("nbody_rr_", "nbody_ragged64_", "nbody_restricted64_", "nbody_ragged_",
                                                  "nbody_restricted_", "nbody_ensemble64_"))]
    assert "RaggedRestrictedEnsemble64" in nb.__all__ and nb.RaggedRestrictedEnsemble64 is nb.ensemble.RaggedRestrictedEnsemble64
    assert C.RR64Handle._prefix == "nbody_rr64" and C.RR64Handle._suffix == "" and C.RR64Handle._dtype is F64
    assert issubclass(C.RR64Handle, C.RRHandle) and C.RRHandle._prefix == "nbody_rr" and C.RRHandle._dtype is F32


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_rr64_has_no_cpu_fallback(nb):
    C = nb._capi
    lib = C.load()
    h = ctypes.c_void_p()
    assert lib.nbody_rr64_create(ctypes.byref(h), 0) == C.ERR_NO_DEVICE and not h.value
    msg = lib.nbody_rr64_last_error(None)
    assert msg and msg.startswith(b"nbody_rr64_create:") and b"no CPU path" in msg
    with pytest.raises(C.NBodyError) as e:
        nb.RaggedRestrictedEnsemble64(*_worlds([2, 4]), tracers=_tracers([5, None]))
    assert e.value.code == C.ERR_NO_DEVICE and "no CPU path" in str(e.value) and "nbody_rr64_create:" in str(e.value)


@pytest.mark.parametrize("which", ["product", "lab"])
def test_null_handle_calls(nb, which):
    C = nb._capi
    lib = C._load(which)
    prm = C.default_params()
    buf = np.zeros(8, F64)
    w = np.ones(4, np.uint32)
    sizes = np.array([1, 3], np.int64)
    counts = np.array([2, 0], np.int64)
    assert lib.nbody_rr64_create(None, 0) == C.ERR_INVALID
    msg = lib.nbody_rr64_last_error(None)
    assert msg and msg.startswith(b"nbody_rr64_create:")
    # a slot of its own: the siblings' failed creates leave it alone, and it leaves theirs alone
    assert lib.nbody_rr_create(None, 0) == C.ERR_INVALID and lib.nbody_ragged64_create(None, 0) == C.ERR_INVALID
    assert lib.nbody_restricted64_create(None, 0) == C.ERR_INVALID
    assert lib.nbody_rr64_last_error(None) == msg

    def others():
        return [lib.nbody_rr_last_error(None), lib.nbody_ragged64_last_error(None), lib.nbody_restricted64_last_error(None)]

    theirs = others()
    assert msg not in theirs and theirs[0].startswith(b"nbody_rr_create:") and theirs[1].startswith(b"nbody_ragged64_create:")
    assert lib.nbody_rr64_create(None, 0) == C.ERR_INVALID
    assert others() == theirs
    assert lib.nbody_rr64_set_params(None, ctypes.byref(prm)) == C.ERR_INVALID
    assert lib.nbody_rr64_get_params(None, ctypes.byref(prm)) == C.ERR_INVALID
    assert lib.nbody_rr64_upload(None, 2, C._ptr(sizes), C._ptr(buf), C._ptr(buf), C._ptr(w)) == C.ERR_INVALID
    assert lib.nbody_rr64_download(None, C._ptr(buf), C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_rr64_tracers_upload(None, 2, C._ptr(counts), C._ptr(buf), C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_rr64_tracers_download(None, C._ptr(buf), C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_rr64_update(None, 0.1, 1, None) == C.ERR_INVALID
    assert lib.nbody_rr64_accel(None, C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_rr64_tracers_accel(None, C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_rr64_sizes(None, C._ptr(sizes), C._ptr(counts)) == C.ERR_INVALID
    assert lib.nbody_rr64_num_worlds(None) == 0 and lib.nbody_rr64_num_rows(None) == 0 and lib.nbody_rr64_num_tracer_rows(None) == 0
    lib.nbody_rr64_destroy(None)
    assert not buf.any() and sizes.tolist() == [1, 3] and counts.tolist() == [2, 0]
    # the plan needs no handle: every output may be NULL, and a refusal names "ragged restricted", goes to this handle's slot and
    # writes nothing
    assert lib.nbody_rr64_plan(2, C._ptr(sizes), C._ptr(counts), None, None, None, None, None) == C.OK
    launch, first = np.full(2, -7, np.int32), np.full(2, -7, np.int64)
    n_launches = ctypes.c_int32(-7)
    lds, blocks = np.full(6, -7, np.int32), np.full(6, -7, np.int64)

    def plan(b, n, m):
        return lib.nbody_rr64_plan(b, None if n is None else C._ptr(n), None if m is None else C._ptr(m), C._ptr(launch), C._ptr(first),
                                   ctypes.byref(n_launches), C._ptr(lds), C._ptr(blocks))

    for bad_n, bad_m in (([0, 3], [2, 0]), ([1, 4097], [2, 0]), ([-1, 3], [2, 0]), ([1, 3], [2, -1]), ([1, 3], [1 << 26, 1])):
        assert plan(2, np.array(bad_n, np.int64), np.array(bad_m, np.int64)) == C.ERR_INVALID, (bad_n, bad_m)
        assert b"ragged restricted" in lib.nbody_rr64_last_error(None)
        assert others() == theirs
    assert plan(0, sizes, counts) == C.ERR_INVALID
    assert plan(2, None, counts) == C.ERR_INVALID
    assert plan(2, sizes, None) == C.ERR_INVALID
    assert launch.tolist() == [-7, -7] and first.tolist() == [-7, -7] and n_launches.value == -7
    assert lds.tolist() == [-7] * 6 and blocks.tolist() == [-7] * 6
    assert plan(2, sizes, counts) == C.OK
    assert launch.tolist() == [0, -1] and first.tolist() == [0, -1] and n_launches.value == 1
    assert lds.tolist() == [160, 0, 0, 0, 0, 0] and blocks.tolist() == [1, 0, 0, 0, 0, 0]       # one body: 8 padded rows of 20 B


# ------------------------------------------------------------------ rejections
def test_rr64_rejects_bad_input_before_any_handle_exists(nb, monkeypatch):
    made = []

    def no_handle(*a, **k):
        made.append(1)
        raise AssertionError("a handle was created")

    monkeypatch.setattr(nb.RaggedRestrictedEnsemble64, "_new_handle", staticmethod(no_handle))
    p, v = _worlds([8, 5, 300])
    w = [np.ones(n, np.uint32) for n in (8, 5, 300)]
    tr = _tracers([4, None, 600])
    z = np.zeros
    bad = [
        dict(positions=_worlds([8, 0, 5])[0], velocities=_worlds([8, 0, 5])[1]),              # a size of 0
        dict(positions=_worlds([8, 4097])[0], velocities=_worlds([8, 4097])[1]),              # a size of 4097
        dict(positions=[], velocities=[]),                                                    # no world
        dict(positions=p, velocities=v[:2]),                                                  # lists of different lengths
        dict(positions=p, velocities=v, weights=w[:2]),
        dict(positions=p, velocities=v, tracers=tr[:2]),
        dict(positions=p, velocities=v, tracers=tr + [None]),
        dict(positions=_worlds([8, 5], F32)[0], velocities=_worlds([8, 5], F32)[1]),          # float32
        dict(positions=p, velocities=[a.astype(F32) for a in v]),
        dict(positions=p, velocities=v, tracers=_tracers([4, None, 600], F32)),
        dict(positions=p, velocities=v, tracers=[tr[0], None, (z((600, 2), F64), z((600, 2), F32))]),
        dict(positions=p, velocities=v, weights=[a.astype(F64) for a in w]),                  # weights are integers
        dict(positions=p, velocities=[v[0], z((6, 2), F64), v[2]]),                           # a velocity of another shape
        dict(positions=p, velocities=v, tracers=[(z((4, 2), F64), z((5, 2), F64)), None, None]),   # a tracer pair of differing shapes
        dict(positions=p, velocities=v, tracers=[(z((4, 3), F64), z((4, 3), F64)), None, None]),   # not x,y
        dict(positions=p, velocities=v, tracers=[z((4, 2), F64), None, None]),                # not a pair
        dict(positions=p, velocities=v, tracers=[(z((4, 2), F64),), None, None]),
        dict(positions=p, velocities=v, tracers=(z((3, 4, 2), F64))),                         # an array where a list belongs
        dict(positions=p[0], velocities=v),
    ]
    for kw in bad:
        with pytest.raises(ValueError, match=r"^RaggedRestrictedEnsemble64: "):
            nb.RaggedRestrictedEnsemble64(**kw)
    # a float32 array is refused with a message that says which class takes it — bodies and tracers alike
    for kw in bad[7:11]:
        with pytest.raises(ValueError, match=r"must be float64 \(got float32\); RaggedRestrictedEnsemble takes float32$"):
            nb.RaggedRestrictedEnsemble64(**kw)
    # sums above 2^26 without a gigabyte of zeros: zero-stride views have the shape and cost nothing
    big = [np.broadcast_to(np.zeros((1, 2), F64), (4096, 2))] * ((1 << 14) + 1)
    with pytest.raises(ValueError, match=r"^RaggedRestrictedEnsemble64: .*2\^26"):
        nb.RaggedRestrictedEnsemble64(big, big)
    half = np.broadcast_to(np.zeros((1, 2), F64), ((1 << 25) + 1, 2))
    with pytest.raises(ValueError, match=r"^RaggedRestrictedEnsemble64: .*tracers.*2\^26"):
        nb.RaggedRestrictedEnsemble64(p, v, tracers=[(half, half), None, (half, half)])
    with pytest.raises(ValueError, match=r"^RaggedRestrictedEnsemble64: arith"):
        nb.RaggedRestrictedEnsemble64(p, v, tracers=tr, arith="double")
    assert not made
    # past the checks the class does ask for a handle: the patch is what the cases above did not reach
    with pytest.raises(AssertionError, match="a handle was created"):
        nb.RaggedRestrictedEnsemble64(p, v, w, tr)
    assert made == [1]


def test_the_f32_class_keeps_its_messages(nb, monkeypatch):
    monkeypatch.setattr(nb.RaggedRestrictedEnsemble, "_new_handle", staticmethod(lambda *a, **k: pytest.fail("a handle was created")))
    p, v = _worlds([8, 5], F32)
    with pytest.raises(ValueError) as e:
        nb.RaggedRestrictedEnsemble(*_worlds([8, 5], F64))
    assert str(e.value) == "RaggedRestrictedEnsemble: world 0: position must be float32 (got float64); it takes float32 only"
    with pytest.raises(ValueError) as e:
        nb.RaggedRestrictedEnsemble(p, v, tracers=_tracers([4, None], F64))
    assert str(e.value) == "RaggedRestrictedEnsemble: world 0: tracer position must be float32 (got float64)"


def test_checked_rr_tracers_takes_the_dtype(nb):
    from nbody_simulation_amd.ensemble import _checked_rr_tracers
    sizes = np.array([3, 1, 9, 2], np.int64)
    tr = [(np.full((5, 2), 1, F64), np.full((5, 2), -1, F64)), None, (np.zeros((0, 2), F64), np.zeros((0, 2), F64)),
          (np.full((7, 2), 4, F64)[::2], np.full((4, 2), -4, F64))]
    counts, tp, tv = _checked_rr_tracers(tr, sizes, "RaggedRestrictedEnsemble64", F64)
    assert counts.dtype == np.int64 and counts.tolist() == [5, 0, 0, 4]
    assert tp.shape == tv.shape == (9, 2) and tp.flags.c_contiguous and tp.dtype == F64 and tv.dtype == F64
    assert tp[:, 0].tolist() == [1.0] * 5 + [4.0] * 4 and np.array_equal(tv, -tp)
    with pytest.raises(ValueError, match=r"^RaggedRestrictedEnsemble: world 0: tracer position must be float32 \(got float64\)$"):
        _checked_rr_tracers(tr, sizes)                                      # the default is the f32 class's
    for none in (None, [None] * 4, [None, None, tr[2], None]):
        counts, tp, tv = _checked_rr_tracers(none, sizes, "RaggedRestrictedEnsemble64", F64)
        assert counts.tolist() == [0, 0, 0, 0] and tp is None and tv is None


# ------------------------------------------------------------------ the plan
def _restated_plan(sizes, counts, lds_of):
    """The tracers' plan as include/nbody_ensemble.h states it -> (launch_of_world, first_block_of_world, lds, blocks, items):
    items[l] is the list of the blocks of launch l, each (world, tracer offset within the world, count)."""
    classes = sorted({_class(n) for n, m in zip(sizes, counts) if m})
    launch_of_class = {c: l for l, c in enumerate(classes)}
    lds = [lds_of(max(n for n, m in zip(sizes, counts) if m and _class(n) == c)) for c in classes]
    items = [[] for _ in classes]
    launch, first = [], []
    for k, (n, m) in enumerate(zip(sizes, counts)):
        if not m:
            launch.append(-1), first.append(-1)
            continue
        l = launch_of_class[_class(n)]
        launch.append(l), first.append(len(items[l]))
        items[l] += [(k, at, min(TILE, m - at)) for at in range(0, m, TILE)]
    return launch, first, lds, [len(i) for i in items], items


def _check_plan(nb, sizes, counts, dtype=F64):
    lds_of = _lds64 if dtype == F64 else _lds32
    plan = nb.rr_plan(sizes, counts, dtype=dtype)
    launch, first, lds, blocks, items = _restated_plan(sizes, counts, lds_of)
    assert plan["launch_of_world"].tolist() == launch and plan["first_block_of_world"].tolist() == first
    assert plan["lds_bytes"].tolist() == lds and plan["blocks"].tolist() == blocks
    assert len(lds) <= 6 and all(b >= 1 for b in blocks)
    # block by block: every tracer of every world in exactly one block of its world's launch, contiguous and ascending
    for k, (n, m) in enumerate(zip(sizes, counts)):
        if not m:
            continue
        l, f = launch[k], first[k]
        mine = items[l][f:f + (m + TILE - 1) // TILE]
        assert [w for w, _, _ in mine] == [k] * len(mine), k
        assert [at for _, at, _ in mine] == list(range(0, m, TILE)) and sum(c for _, _, c in mine) == m, k
        assert all(1 <= c <= TILE for _, _, c in mine) and lds[l] >= lds_of(n), k
        assert f == 0 or items[l][f - 1][0] < k, k                         # world order inside a launch
    assert sum(blocks) == sum((m + TILE - 1) // TILE for m in counts)
    return plan


def test_plan_under_the_f64_lds_block_by_block_against_the_restatement(nb):
    assert [_lds64(n) for n in (1, 8, 9, 3272, 3273, 4096)] == [160, 160, 320, 65440, 65600, 81920]
    rng = np.random.default_rng(20261021)
    pairs = [(n, m) for n in PLAN_N for m in PLAN_M]
    order = rng.permutation(len(pairs))
    sizes, counts = [pairs[i][0] for i in order], [pairs[i][1] for i in order]
    plan = _check_plan(nb, sizes, counts)
    assert plan["lds_bytes"].tolist() == [_lds64(n) for n in CAPS]         # every class launches, each under its cap's LDS
    assert (plan["launch_of_world"][np.array(counts) == 0] == -1).all() and (plan["first_block_of_world"][np.array(counts) == 0] == -1).all()
    assert (plan["launch_of_world"][np.array(counts) > 0] >= 0).all()
    # the same worlds under float32: the f32 plan, as before — and as the default
    p32 = _check_plan(nb, sizes, counts, dtype=F32)
    default = nb.rr_plan(sizes, counts)
    assert all(np.array_equal(default[k], p32[k]) for k in p32)
    assert p32["lds_bytes"].tolist() == [_lds32(n) for n in CAPS] and p32["blocks"].tolist() == plan["blocks"].tolist()
    assert p32["launch_of_world"].tolist() == plan["launch_of_world"].tolist()   # the classes are by n, whatever the precision
    # every n with every m on its own, and in a pair with a world without tracers on either side
    for n in PLAN_N:
        for m in PLAN_M:
            p = _check_plan(nb, [n], [m])
            assert p["blocks"].tolist() == ([(m + 511) // 512] if m else []) and p["lds_bytes"].tolist() == ([_lds64(n)] if m else [])
            _check_plan(nb, [4096, n, 1], [0, m, 0])
    # a class launches under the LDS of its largest world WITH tracers; a class whose worlds have none does not launch
    p = _check_plan(nb, [200, 150, 130, 7, 1000], [0, 5, 700, 0, 513])
    assert p["lds_bytes"].tolist() == [_lds64(150), _lds64(1000)] and p["blocks"].tolist() == [3, 2]
    assert p["launch_of_world"].tolist() == [-1, 0, 0, -1, 1] and p["first_block_of_world"].tolist() == [-1, 0, 1, -1, 0]
    p = _check_plan(nb, [4096, 3273, 3272, 7], [0, 0, 513, 1])             # the largest world of the last class has no tracers ...
    assert p["lds_bytes"].tolist() == [160, 65440] and p["blocks"].tolist() == [1, 2]   # ... nor the next: under 64 KB
    p = _check_plan(nb, [4096, 3273, 3272, 7], [0, 1, 513, 1])
    assert p["lds_bytes"].tolist() == [160, 65600] and p["blocks"].tolist() == [1, 3]   # above it
    p = _check_plan(nb, [200, 7], [0, 0])
    assert p["lds_bytes"].tolist() == [] and p["blocks"].tolist() == [] and p["launch_of_world"].tolist() == [-1, -1]
    # 10^4 worlds of random sizes and counts, a third without tracers
    n = rng.integers(1, 4097, 10_000)
    m = np.where(rng.integers(0, 3, 10_000) == 0, 0, rng.integers(0, 3000, 10_000))
    _check_plan(nb, [int(x) for x in n], [int(x) for x in m])


def test_plan_refuses_sizes_counts_and_dtypes_outside_the_limits(nb):
    C = nb._capi
    for bad_n, bad_m in (([], []), ([0], [1]), ([4097], [1]), ([5, -1], [1, 1]), ([5, 5], [1, -1]), ([5, 5], [1]), ([5], [1, 1])):
        with pytest.raises(ValueError):
            nb.rr_plan(bad_n, bad_m, dtype=F64)
    with pytest.raises(ValueError, match="2\\^26"):
        nb.rr_plan([5, 5], [1 << 26, 1], dtype=F64)
    for dtype in (np.float16, np.int64):
        with pytest.raises(ValueError, match="rr_plan: dtype must be float32 or float64"):
            nb.rr_plan([5], [1], dtype=dtype)
    with pytest.raises(C.NBodyError) as e:
        C.rr_plan([5, 5], [1 << 26, 1], f64=True)
    assert e.value.code == C.ERR_INVALID and "ragged restricted" in str(e.value) and "2^26" in str(e.value)
    launch, first, lds, blocks = C.rr_plan([5, 5], [1 << 26, 0], f64=True)   # 2^26 exactly
    assert blocks.tolist() == [1 << 17] and launch.tolist() == [0, -1] and lds.tolist() == [160]
