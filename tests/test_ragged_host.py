"""Ragged ensembles (nbody_ragged_*, nb.RaggedEnsemble, nb.ragged_plan) without a GPU: argument checks that must fire before any
handle exists, the refusal to run without a device, NULL-handle calls, the declared names in both libraries, and the launch plan
— which is pure host code — checked block by block."""
import ctypes
import os
import re

import numpy as np
import pytest

F32 = np.float32
NAMES = ["nbody_ragged_" + s for s in ("create", "destroy", "last_error", "set_params", "get_params", "upload_f32", "download_f32",
                                       "num_worlds", "num_rows", "sizes", "update_f32", "accel_f32", "plan")]
PLAN_SIZES = [1, 2, 3, 7, 12, 24, 50, 100, 128, 129, 256, 257, 300, 512, 513, 1000, 1024, 1025, 2048, 2049, 4096]
CAPS = (128, 256, 512, 1024, 2048, 4096)


def _worlds(sizes, dtype=F32):
    return [np.zeros((n, 2), dtype) for n in sizes], [np.zeros((n, 2), dtype) for n in sizes]


# what the uniform ensemble does for a world of n bodies (csrc/ensemble_shape.h), restated
def _split(n):
    if n > 128:
        return 1
    split, targets = 2, 128
    while targets // 2 >= n and split < 64:
        targets //= 2
        split *= 2
    return split


def _tiles(n):
    tpb = 256 // _split(n)
    return (n + tpb - 1) // tpb


def _lds(n):
    return (n + 1) // 2 * 24


def _class(n):
    return next(c for c, cap in enumerate(CAPS) if n <= cap)


# ------------------------------------------------------------------ rejections
def test_ragged_rejects_bad_input_before_any_handle_exists(nb, monkeypatch):
    C = nb._capi
    made = []
    monkeypatch.setattr(C, "RaggedHandle", lambda *a, **k: made.append(1) or pytest.fail("a handle was created"))
    p, v = _worlds([8, 5, 300])
    w = [np.ones(n, np.uint32) for n in (8, 5, 300)]
    bad = [
        (*_worlds([8, 0, 5]), None),                                       # a size of 0
        (*_worlds([8, 4097]), None),                                       # a size of 4097
        ([], [], None),                                                    # no world
        (p, v[:2], None),                                                  # lists of different lengths
        (p, v, w[:2]),
        (*_worlds([8, 5], np.float64), None),                              # float64
        (p, [a.astype(np.float64) for a in v], None),
        (p, v, [a.astype(F32) for a in w]),                                # weights are integers
        (p, v, [w[0], np.ones(4, np.uint32), w[2]]),                       # a weight of the wrong length
        (p, [v[0], np.zeros((6, 2), F32), v[2]], None),                    # a velocity of another shape
        ([np.zeros((8, 3), F32)], [np.zeros((8, 3), F32)], None),          # not x,y
        (p[0], v, None),                                                   # an array where a list of worlds belongs
    ]
    for pos, vel, wgt in bad:
        with pytest.raises(ValueError):
            nb.RaggedEnsemble(pos, vel, wgt)
    # more than 2^26 rows, without 512 MB of zeros: broadcast views have the shape and cost nothing
    big = [np.broadcast_to(np.zeros((1, 2), F32), (4096, 2))] * ((1 << 14) + 1)
    with pytest.raises(ValueError, match="2\\^26"):
        nb.RaggedEnsemble(big, big)
    with pytest.raises(ValueError):
        nb.RaggedEnsemble(p, v, arith="double")
    assert not made


def test_checked_ragged_lays_the_rows_out_in_world_order(nb):
    from nbody_simulation_amd.ensemble import _checked_ragged
    sizes = [3, 1, 4096, 2]
    pos = [np.full((n, 2), k, F32) for k, n in enumerate(sizes)]
    vel = [np.full((n, 2), -k, F32) for k, n in enumerate(sizes)]
    wgt = [np.full(n, k + 1, np.int64) for k, n in enumerate(sizes)]
    s, p, v, w = _checked_ragged(pos, vel, wgt)
    assert s.dtype == np.int64 and s.tolist() == sizes
    assert p.shape == v.shape == (sum(sizes), 2) and p.dtype == v.dtype == F32 and w.dtype == np.uint32 and w.shape == (sum(sizes),)
    assert p[:, 0].tolist() == sum(([float(k)] * n for k, n in enumerate(sizes)), [])
    assert w.tolist() == sum(([k + 1] * n for k, n in enumerate(sizes)), []) and np.array_equal(v, -p)
    assert _checked_ragged(pos, vel, None)[3] is None


# ------------------------------------------------------------------ handle-free calls
@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_ragged_has_no_cpu_fallback(nb):
    C = nb._capi
    lib = C.load()
    h = ctypes.c_void_p()
    assert lib.nbody_ragged_create(ctypes.byref(h), 0) == C.ERR_NO_DEVICE and not h.value
    msg = lib.nbody_ragged_last_error(None)
    assert msg and b"no CPU path" in msg and b"nbody_ragged_create" in msg
    with pytest.raises(C.NBodyError) as e:
        nb.RaggedEnsemble(*_worlds([2, 4]))
    assert e.value.code == C.ERR_NO_DEVICE and "no CPU path" in str(e.value)


@pytest.mark.parametrize("which", ["product", "lab"])
def test_null_handle_calls(nb, which):
    C = nb._capi
    lib = C._load(which)
    prm = C.default_params()
    buf = np.zeros(8, F32)
    w = np.ones(4, np.uint32)
    sizes = np.array([1, 3], np.int64)
    assert lib.nbody_ragged_create(None, 0) == C.ERR_INVALID and lib.nbody_ragged_last_error(None)
    assert lib.nbody_ragged_set_params(None, ctypes.byref(prm)) == C.ERR_INVALID
    assert lib.nbody_ragged_get_params(None, ctypes.byref(prm)) == C.ERR_INVALID
    assert lib.nbody_ragged_upload_f32(None, 2, C._ptr(sizes), C._ptr(buf), C._ptr(buf), C._ptr(w)) == C.ERR_INVALID
    assert lib.nbody_ragged_download_f32(None, C._ptr(buf), C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_ragged_update_f32(None, 0.1, 1, None) == C.ERR_INVALID
    assert lib.nbody_ragged_accel_f32(None, C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_ragged_sizes(None, C._ptr(sizes)) == C.ERR_INVALID
    assert lib.nbody_ragged_num_worlds(None) == 0 and lib.nbody_ragged_num_rows(None) == 0
    lib.nbody_ragged_destroy(None)
    assert not buf.any() and sizes.tolist() == [1, 3]
    # the plan needs no handle: every output may be NULL, and bad sizes are refused with a message that names "ragged"
    assert lib.nbody_ragged_plan(2, C._ptr(sizes), None, None, None, None, None) == C.OK
    launch = np.full(2, -7, np.int32)
    for bad in ([0, 3], [1, 4097], [-1, 3]):
        b = np.array(bad, np.int64)
        assert lib.nbody_ragged_plan(2, C._ptr(b), C._ptr(launch), None, None, None, None) == C.ERR_INVALID
        assert b"ragged" in lib.nbody_ragged_last_error(None)
    assert lib.nbody_ragged_plan(0, C._ptr(sizes), C._ptr(launch), None, None, None, None) == C.ERR_INVALID
    assert lib.nbody_ragged_plan(2, None, C._ptr(launch), None, None, None, None) == C.ERR_INVALID
    assert launch.tolist() == [-7, -7]                                     # nothing was written


def test_header_declares_the_ragged_calls_and_both_libraries_export_them(nb):
    C = nb._capi
    declared = C.declared_symbols()
    assert set(NAMES) <= set(declared) and set(NAMES) <= set(C._SIGS)
    assert sorted(s for s in declared if s.startswith("nbody_ragged_")) == sorted(NAMES)
    assert sorted(s for s in C._SIGS if s.startswith("nbody_ragged_")) == sorted(NAMES)
    for path in (C.LIB_PATH, C.LAB_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in NAMES if not hasattr(lib, s)], path
    with open(C.HEADER_PATH) as f:
        head = f.read()
    assert int(re.search(r"#define\s+NBODY_ABI_VERSION\s+(\d+)", head).group(1)) == 3    # new symbols only
    with open(os.path.join(os.path.dirname(C.HEADER_PATH), "nbody_ensemble.h")) as f:
        ens = f.read()
    assert "typedef struct nbody_ragged nbody_ragged;" in ens
    assert int(re.search(r"#define\s+NBODY_RAGGED_MAX_LAUNCHES\s+(\d+)", ens).group(1)) == C.RAGGED_MAX_LAUNCHES == 6
    assert nb.RaggedEnsemble is nb.ensemble.RaggedEnsemble and nb.ragged_plan is nb.ensemble.ragged_plan
    assert C.RaggedHandle._prefix == "nbody_ragged"


# ------------------------------------------------------------------ the plan
def _check_plan(nb, sizes):
    """Every property of the plan of these sizes; -> the plan."""
    plan = nb.ragged_plan(sizes)
    launch, first = plan["launch_of_world"], plan["first_block_of_world"]
    lds, blocks = plan["lds_bytes"], plan["blocks"]
    n_launches = len(lds)
    assert 1 <= n_launches <= 6 and len(blocks) == n_launches and len(launch) == len(first) == len(sizes)
    assert launch.min() >= 0 and launch.max() == n_launches - 1
    owner = [np.full(int(b), -1, np.int64) for b in blocks]               # which world every block of every launch belongs to
    for k, n in enumerate(sizes):
        l, f, t = int(launch[k]), int(first[k]), _tiles(n)
        assert 0 <= f and f + t <= blocks[l], (k, n)
        assert (owner[l][f:f + t] == -1).all(), f"world {k}: its blocks overlap another world's"
        owner[l][f:f + t] = k                                              # tiles 0 .. t-1 are blocks f .. f+t-1: contiguous
    for l in range(n_launches):
        assert (owner[l] >= 0).all(), f"launch {l} has blocks of no world"  # with the above: every (world, tile) exactly once
        members = [n for k, n in enumerate(sizes) if launch[k] == l]
        assert members and len({_class(n) for n in members}) == 1, l       # one class per launch
        assert lds[l] == _lds(max(members)) and all(lds[l] >= _lds(n) for n in members), l
        assert max(members) <= 128 or lds[l] <= 2 * min(_lds(n) for n in members) + 24, l
        # worlds follow one another in world order inside a launch
        order = [k for k in range(len(sizes)) if launch[k] == l]
        assert [int(first[k]) for k in order] == sorted(int(first[k]) for k in order), l
    classes = [_class([n for k, n in enumerate(sizes) if launch[k] == l][0]) for l in range(n_launches)]
    assert classes == sorted(set(_class(n) for n in sizes))                # every class that has a world, in size order
    assert int(blocks.sum()) == sum(_tiles(n) for n in sizes)
    return plan


def test_plan_covers_every_world_and_tile_exactly_once(nb):
    rng = np.random.default_rng(20261019)
    sizes = PLAN_SIZES * 3 + [128, 129, 4096, 1]
    sizes = [int(n) for n in rng.permutation(sizes)]
    plan = _check_plan(nb, sizes)
    assert len(plan["lds_bytes"]) == 6
    assert plan["lds_bytes"].tolist() == [_lds(128), _lds(256), _lds(512), _lds(1024), _lds(2048), _lds(4096)]
    assert plan["lds_bytes"][0] <= 1536                                    # every lane split sits under 1.5 KB
    # classes without a world launch nothing, and the LDS is that of the largest member, not of the class cap
    plan = _check_plan(nb, [300, 7, 1000, 12, 290])
    assert plan["lds_bytes"].tolist() == [_lds(12), _lds(300), _lds(1000)] and plan["blocks"].tolist() == [2, 4, 4]
    assert plan["launch_of_world"].tolist() == [1, 0, 2, 0, 1] and plan["first_block_of_world"].tolist() == [0, 0, 0, 1, 2]
    # 10^4 worlds of random sizes
    _check_plan(nb, [int(n) for n in rng.integers(1, 4097, 10_000)])


@pytest.mark.parametrize("n", [1, 5, 64, 128, 129, 300, 1024, 4096])
def test_plan_of_equal_sizes_is_the_uniform_launch(nb, n):
    for b in (1, 5):
        plan = _check_plan(nb, [n] * b)
        assert plan["lds_bytes"].tolist() == [_lds(n)] and plan["blocks"].tolist() == [b * _tiles(n)]
        assert plan["launch_of_world"].tolist() == [0] * b
        assert plan["first_block_of_world"].tolist() == [k * _tiles(n) for k in range(b)]
    assert _tiles(1) == 1 and _tiles(4096) == 16 and _lds(1) == 24 and _lds(4096) == 49152


def test_plan_restatement_matches_the_split_ranges(nb):
    """The restatement above against the ranges the kernels document: 64 lanes per target up to 4 bodies, then 32, 16, 8, 4, 2,
    and one target per lane above 128; at most 16 tiles."""
    want = {1: 64, 4: 64, 5: 32, 8: 32, 9: 16, 16: 16, 17: 8, 32: 8, 33: 4, 64: 4, 65: 2, 128: 2, 129: 1, 4096: 1}
    assert {n: _split(n) for n in want} == want
    assert max(_tiles(n) for n in range(1, 4097)) == 16 and all(_tiles(n) == 1 for n in range(1, 129))


def test_plan_refuses_sizes_outside_the_limits(nb):
    C = nb._capi
    for bad in ([], [0], [4097], [5, -1]):
        with pytest.raises(ValueError):
            nb.ragged_plan(bad)
    with pytest.raises(C.NBodyError) as e:
        C.ragged_plan([4096] * ((1 << 14) + 1))                            # 2^26 + 4096 rows
    assert e.value.code == C.ERR_INVALID and "ragged" in str(e.value) and "2^26" in str(e.value)
    C.ragged_plan([4096] * (1 << 14))                                      # 2^26 exactly
