"""Ragged restricted ensembles (nbody_rr_*, nb.RaggedRestrictedEnsemble, nb.rr_plan) without a GPU: the declared names in both
libraries, the refusal to run without a device, NULL-handle calls with an error slot of their own, argument checks that must
fire before any handle exists, and the tracers' launch plan — which is pure host code — checked block by block against a
restatement."""
import ctypes
import os
import re

import numpy as np
import pytest

F32 = np.float32
# the seventeen calls the header lists; with NBODY_RR_MAX_LAUNCHES the section defines eighteen names
NAMES = ["nbody_rr_" + s for s in ("create", "destroy", "last_error", "set_params", "get_params", "upload_f32", "download_f32",
                                   "tracers_upload_f32", "tracers_download_f32", "num_worlds", "num_rows", "num_tracer_rows",
                                   "sizes", "update_f32", "accel_f32", "tracers_accel_f32", "plan")]
PLAN_N = [1, 2, 7, 65, 128, 129, 256, 257, 1000, 2049, 4096]
PLAN_M = [0, 1, 511, 512, 513, 1025]
CAPS = (128, 256, 512, 1024, 2048, 4096)
TILE = 512


def _worlds(sizes, dtype=F32):
    return [np.zeros((n, 2), dtype) for n in sizes], [np.zeros((n, 2), dtype) for n in sizes]


def _tracers(counts, dtype=F32):
    return [None if m is None else (np.zeros((m, 2), dtype), np.zeros((m, 2), dtype)) for m in counts]


def _lds(n):
    return (n + 1) // 2 * 24


def _class(n):
    return next(c for c, cap in enumerate(CAPS) if n <= cap)


# ------------------------------------------------------------------ names
def test_header_declares_the_rr_calls_and_both_libraries_export_them(nb):
    C = nb._capi
    assert len(NAMES) == 17
    declared = C.declared_symbols()
    assert sorted(s for s in declared if s.startswith("nbody_rr_")) == sorted(NAMES)
    assert sorted(s for s in C._SIGS if s.startswith("nbody_rr_")) == sorted(NAMES)
    assert sorted(C._SIGS) == declared
    for path in (C.LIB_PATH, C.LAB_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in NAMES if not hasattr(lib, s)], path
    with open(C.HEADER_PATH) as f:
        head = f.read()
    assert int(re.search(r"#define\s+NBODY_ABI_VERSION\s+(\d+)", head).group(1)) == 3 == C.ABI_VERSION    # new symbols only
    assert "nbody_rr" not in head                                           # declared in nbody_ensemble.h, which it includes
    with open(os.path.join(os.path.dirname(C.HEADER_PATH), "nbody_ensemble.h")) as f:
        ens = f.read()
    assert "typedef struct nbody_rr nbody_rr;" in ens
    assert int(re.search(r"#define\s+NBODY_RR_MAX_LAUNCHES\s+(\d+)", ens).group(1)) == C.RR_MAX_LAUNCHES == 12
    # the prefix is its own: no call of this handle falls into the closed sets of the ragged or the restricted handle
    assert not [s for s in NAMES if s.startswith(("nbody_ragged_", "nbody_restricted_", "nbody_ensemble_"))]
    assert "RaggedRestrictedEnsemble" in nb.__all__ and nb.RaggedRestrictedEnsemble is nb.ensemble.RaggedRestrictedEnsemble
    assert "rr_plan" in nb.__all__ and nb.rr_plan is nb.ensemble.rr_plan
    assert C.RRHandle._prefix == "nbody_rr"


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_rr_has_no_cpu_fallback(nb):
    C = nb._capi
    lib = C.load()
    h = ctypes.c_void_p()
    assert lib.nbody_rr_create(ctypes.byref(h), 0) == C.ERR_NO_DEVICE and not h.value
    msg = lib.nbody_rr_last_error(None)
    assert msg and msg.startswith(b"nbody_rr_create:") and b"no CPU path" in msg
    with pytest.raises(C.NBodyError) as e:
        nb.RaggedRestrictedEnsemble(*_worlds([2, 4]), tracers=_tracers([5, None]))
    assert e.value.code == C.ERR_NO_DEVICE and "no CPU path" in str(e.value)


@pytest.mark.parametrize("which", ["product", "lab"])
def test_null_handle_calls(nb, which):
    C = nb._capi
    lib = C._load(which)
    prm = C.default_params()
    buf = np.zeros(8, F32)
    w = np.ones(4, np.uint32)
    sizes = np.array([1, 3], np.int64)
    counts = np.array([2, 0], np.int64)
    assert lib.nbody_rr_create(None, 0) == C.ERR_INVALID
    msg = lib.nbody_rr_last_error(None)
    assert msg and msg.startswith(b"nbody_rr_create:")
    # a slot of its own: the other handles' failed creates leave it alone, and it leaves theirs alone
    assert lib.nbody_ensemble_create(None, 0) == C.ERR_INVALID and lib.nbody_ragged_create(None, 0) == C.ERR_INVALID
    assert lib.nbody_restricted_create(None, 0) == C.ERR_INVALID
    assert lib.nbody_rr_last_error(None) == msg
    others = [lib.nbody_ensemble_last_error(None), lib.nbody_ragged_last_error(None), lib.nbody_restricted_last_error(None)]
    assert msg not in others
    assert lib.nbody_rr_create(None, 0) == C.ERR_INVALID
    assert [lib.nbody_ensemble_last_error(None), lib.nbody_ragged_last_error(None), lib.nbody_restricted_last_error(None)] == others
    assert lib.nbody_rr_set_params(None, ctypes.byref(prm)) == C.ERR_INVALID
    assert lib.nbody_rr_get_params(None, ctypes.byref(prm)) == C.ERR_INVALID
    assert lib.nbody_rr_upload_f32(None, 2, C._ptr(sizes), C._ptr(buf), C._ptr(buf), C._ptr(w)) == C.ERR_INVALID
    assert lib.nbody_rr_download_f32(None, C._ptr(buf), C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_rr_tracers_upload_f32(None, 2, C._ptr(counts), C._ptr(buf), C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_rr_tracers_download_f32(None, C._ptr(buf), C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_rr_update_f32(None, 0.1, 1, None) == C.ERR_INVALID
    assert lib.nbody_rr_accel_f32(None, C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_rr_tracers_accel_f32(None, C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_rr_sizes(None, C._ptr(sizes), C._ptr(counts)) == C.ERR_INVALID
    assert lib.nbody_rr_num_worlds(None) == 0 and lib.nbody_rr_num_rows(None) == 0 and lib.nbody_rr_num_tracer_rows(None) == 0
    lib.nbody_rr_destroy(None)
    assert not buf.any() and sizes.tolist() == [1, 3] and counts.tolist() == [2, 0]
    # the plan needs no handle: every output may be NULL, and a refusal names "ragged restricted" and writes nothing
    assert lib.nbody_rr_plan(2, C._ptr(sizes), C._ptr(counts), None, None, None, None, None) == C.OK
    launch, first = np.full(2, -7, np.int32), np.full(2, -7, np.int64)
    n_launches = ctypes.c_int32(-7)
    lds, blocks = np.full(6, -7, np.int32), np.full(6, -7, np.int64)

    def plan(b, n, m):
        return lib.nbody_rr_plan(b, None if n is None else C._ptr(n), None if m is None else C._ptr(m), C._ptr(launch), C._ptr(first),
                                 ctypes.byref(n_launches), C._ptr(lds), C._ptr(blocks))

    for bad_n, bad_m in (([0, 3], [2, 0]), ([1, 4097], [2, 0]), ([-1, 3], [2, 0]), ([1, 3], [2, -1]), ([1, 3], [1 << 26, 1])):
        assert plan(2, np.array(bad_n, np.int64), np.array(bad_m, np.int64)) == C.ERR_INVALID, (bad_n, bad_m)
        assert b"ragged restricted" in lib.nbody_rr_last_error(None)
    assert plan(0, sizes, counts) == C.ERR_INVALID
    assert plan(2, None, counts) == C.ERR_INVALID
    assert plan(2, sizes, None) == C.ERR_INVALID
    assert launch.tolist() == [-7, -7] and first.tolist() == [-7, -7] and n_launches.value == -7
    assert lds.tolist() == [-7] * 6 and blocks.tolist() == [-7] * 6
    assert plan(2, sizes, counts) == C.OK
    assert launch.tolist() == [0, -1] and first.tolist() == [0, -1] and n_launches.value == 1
    assert lds.tolist() == [24, 0, 0, 0, 0, 0] and blocks.tolist() == [1, 0, 0, 0, 0, 0]


# ------------------------------------------------------------------ rejections
def test_rr_rejects_bad_input_before_any_handle_exists(nb, monkeypatch):
    C = nb._capi
    made = []
    monkeypatch.setattr(C, "RRHandle", lambda *a, **k: made.append(1) or pytest.fail("a handle was created"))
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
        dict(positions=_worlds([8, 5], np.float64)[0], velocities=_worlds([8, 5], np.float64)[1]),   # float64
        dict(positions=p, velocities=[a.astype(np.float64) for a in v]),
        dict(positions=p, velocities=v, tracers=_tracers([4, None, 600], np.float64)),
        dict(positions=p, velocities=v, tracers=[tr[0], None, (z((600, 2), F32), z((600, 2), np.float64))]),
        dict(positions=p, velocities=v, weights=[a.astype(F32) for a in w]),                  # weights are integers
        dict(positions=p, velocities=[v[0], z((6, 2), F32), v[2]]),                           # a velocity of another shape
        dict(positions=p, velocities=v, tracers=[(z((4, 2), F32), z((5, 2), F32)), None, None]),   # a tracer pair of differing shapes
        dict(positions=p, velocities=v, tracers=[(z((4, 3), F32), z((4, 3), F32)), None, None]),   # not x,y
        dict(positions=p, velocities=v, tracers=[z((4, 2), F32), None, None]),                # not a pair
        dict(positions=p, velocities=v, tracers=[(z((4, 2), F32),), None, None]),
        dict(positions=p, velocities=v, tracers=(z((3, 4, 2), F32))),                         # an array where a list belongs
        dict(positions=p[0], velocities=v),
    ]
    for kw in bad:
        with pytest.raises(ValueError, match="RaggedRestrictedEnsemble"):
            nb.RaggedRestrictedEnsemble(**kw)
    # sums above 2^26 without 512 MB of zeros: zero-stride views have the shape and cost nothing
    big = [np.broadcast_to(np.zeros((1, 2), F32), (4096, 2))] * ((1 << 14) + 1)
    with pytest.raises(ValueError, match=r"RaggedRestrictedEnsemble.*2\^26"):
        nb.RaggedRestrictedEnsemble(big, big)
    half = np.broadcast_to(np.zeros((1, 2), F32), ((1 << 25) + 1, 2))
    with pytest.raises(ValueError, match=r"RaggedRestrictedEnsemble.*tracers.*2\^26"):
        nb.RaggedRestrictedEnsemble(p, v, tracers=[(half, half), None, (half, half)])
    with pytest.raises(ValueError, match="RaggedRestrictedEnsemble"):
        nb.RaggedRestrictedEnsemble(p, v, tracers=tr, arith="double")
    assert not made


def test_checked_rr_tracers_lays_the_rows_out_in_world_order(nb):
    from nbody_simulation_amd.ensemble import _checked_rr_tracers
    sizes = np.array([3, 1, 9, 2], np.int64)
    tr = [(np.full((5, 2), 1, F32), np.full((5, 2), -1, F32)), None, (np.zeros((0, 2), F32), np.zeros((0, 2), F32)),
          (np.full((7, 2), 4, F32)[::2], np.full((4, 2), -4, F32))]
    counts, tp, tv = _checked_rr_tracers(tr, sizes)
    assert counts.dtype == np.int64 and counts.tolist() == [5, 0, 0, 4]
    assert tp.shape == tv.shape == (9, 2) and tp.flags.c_contiguous and tp.dtype == F32
    assert tp[:, 0].tolist() == [1.0] * 5 + [4.0] * 4 and np.array_equal(tv, -tp)
    for none in (None, [None] * 4, [None, None, tr[2], None]):
        counts, tp, tv = _checked_rr_tracers(none, sizes)
        assert counts.tolist() == [0, 0, 0, 0] and tp is None and tv is None


# ------------------------------------------------------------------ the plan
def _restated_plan(sizes, counts):
    """The tracers' plan as include/nbody_ensemble.h states it -> (launch_of_world, first_block_of_world, lds, blocks, items):
    items[l] is the list of the blocks of launch l, each (world, tracer offset within the world, count)."""
    classes = sorted({_class(n) for n, m in zip(sizes, counts) if m})
    launch_of_class = {c: l for l, c in enumerate(classes)}
    lds = [_lds(max(n for n, m in zip(sizes, counts) if m and _class(n) == c)) for c in classes]
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


def _check_plan(nb, sizes, counts):
    plan = nb.rr_plan(sizes, counts)
    launch, first, lds, blocks, items = _restated_plan(sizes, counts)
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
        assert all(1 <= c <= TILE for _, _, c in mine) and lds[l] >= _lds(n), k
        assert f == 0 or items[l][f - 1][0] < k, k                         # world order inside a launch
    assert sum(blocks) == sum((m + TILE - 1) // TILE for m in counts)
    return plan


def test_plan_block_by_block_against_the_restatement(nb):
    rng = np.random.default_rng(20261020)
    pairs = [(n, m) for n in PLAN_N for m in PLAN_M]
    order = rng.permutation(len(pairs))
    sizes, counts = [pairs[i][0] for i in order], [pairs[i][1] for i in order]
    plan = _check_plan(nb, sizes, counts)
    # (no size of PLAN_N lies in 1025 .. 2048: five of the six classes launch, 2049 and 4096 share the last)
    assert plan["lds_bytes"].tolist() == [_lds(n) for n in (128, 256, 257, 1000, 4096)]
    assert (plan["launch_of_world"][np.array(counts) == 0] == -1).all() and (plan["first_block_of_world"][np.array(counts) == 0] == -1).all()
    assert (plan["launch_of_world"][np.array(counts) > 0] >= 0).all()
    # every n with every m on its own, and in a pair with a world without tracers on either side
    for n in PLAN_N:
        for m in PLAN_M:
            p = _check_plan(nb, [n], [m])
            assert p["blocks"].tolist() == ([(m + 511) // 512] if m else []) and p["lds_bytes"].tolist() == ([_lds(n)] if m else [])
            _check_plan(nb, [4096, n, 1], [0, m, 0])
    # a class launches under the LDS of its largest world WITH tracers; a class whose worlds have none does not launch
    p = _check_plan(nb, [200, 150, 130, 7, 1000], [0, 5, 700, 0, 513])
    assert p["lds_bytes"].tolist() == [_lds(150), _lds(1000)] and p["blocks"].tolist() == [3, 2]
    assert p["launch_of_world"].tolist() == [-1, 0, 0, -1, 1] and p["first_block_of_world"].tolist() == [-1, 0, 1, -1, 0]
    p = _check_plan(nb, [200, 7], [0, 0])
    assert p["lds_bytes"].tolist() == [] and p["blocks"].tolist() == [] and p["launch_of_world"].tolist() == [-1, -1]
    # 10^4 worlds of random sizes and counts, a third without tracers
    n = rng.integers(1, 4097, 10_000)
    m = np.where(rng.integers(0, 3, 10_000) == 0, 0, rng.integers(0, 3000, 10_000))
    _check_plan(nb, [int(x) for x in n], [int(x) for x in m])


def test_plan_refuses_sizes_and_counts_outside_the_limits(nb):
    C = nb._capi
    for bad_n, bad_m in (([], []), ([0], [1]), ([4097], [1]), ([5, -1], [1, 1]), ([5, 5], [1, -1]), ([5, 5], [1]), ([5], [1, 1])):
        with pytest.raises(ValueError):
            nb.rr_plan(bad_n, bad_m)
    with pytest.raises(ValueError, match="2\\^26"):
        nb.rr_plan([5, 5], [1 << 26, 1])
    with pytest.raises(C.NBodyError) as e:
        C.rr_plan([5, 5], [1 << 26, 1])
    assert e.value.code == C.ERR_INVALID and "ragged restricted" in str(e.value) and "2^26" in str(e.value)
    with pytest.raises(C.NBodyError) as e:
        C.rr_plan([4096] * ((1 << 14) + 1), [0] * ((1 << 14) + 1))           # 2^26 + 4096 body rows
    assert e.value.code == C.ERR_INVALID and "ragged restricted" in str(e.value) and "2^26" in str(e.value)
    launch, first, lds, blocks = C.rr_plan([5, 5], [1 << 26, 0])             # 2^26 exactly
    assert blocks.tolist() == [1 << 17] and launch.tolist() == [0, -1]
