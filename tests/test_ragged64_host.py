"""Ragged ensembles in f64 (nbody_ragged64_*, nb.RaggedEnsemble64, nb.ragged_plan(sizes, dtype=float64)) without a GPU: argument
checks that must fire before any handle exists, the refusal to run without a device, NULL-handle calls, the create-error slots,
the declared names in both libraries, and the f64 launch plan — pure host code — checked block by block with the checker of
tests/test_ragged_host.py under the f64 LDS function."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import test_ragged_host as f32_host
from tests.test_ragged_host import CAPS, PLAN_SIZES, _tiles

F32, F64 = np.float32, np.float64
NAMES = ["nbody_ragged64_" + s for s in ("create", "destroy", "last_error", "set_params", "get_params", "upload", "download",
                                         "num_worlds", "num_rows", "sizes", "update", "accel", "plan")]


def _worlds(sizes, dtype=F64):
    return [np.zeros((n, 2), dtype) for n in sizes], [np.zeros((n, 2), dtype) for n in sizes]


# what the f64 ensemble stages for a world of n bodies (csrc/ensemble_shape.h), restated: rows padded to the term block of 8,
# a double2 and a u32 each
def _lds64(n):
    return (n + 7) // 8 * 8 * 20


# ------------------------------------------------------------------ rejections
def test_ragged64_rejects_bad_input_before_any_handle_exists(nb, monkeypatch):
    C = nb._capi
    made = []
    monkeypatch.setattr(C, "Ragged64Handle", lambda *a, **k: made.append(1) or pytest.fail("a handle was created"))
    monkeypatch.setattr(C, "RaggedHandle", lambda *a, **k: made.append(1) or pytest.fail("an f32 handle was created"))
    p, v = _worlds([8, 5, 300])
    w = [np.ones(n, np.uint32) for n in (8, 5, 300)]
    bad = [
        (*_worlds([8, 5], F32), None),                                     # float32: that is nb.RaggedEnsemble's
        (p, [a.astype(F32) for a in v], None),                             # mixed dtypes
        ([a.astype(F32) for a in p], v, None),
        (p[:2] + [p[2].astype(F32)], v, None),                             # one world of another dtype
        (*_worlds([8, 0, 5]), None),                                       # a size of 0
        (*_worlds([8, 4097]), None),                                       # a size of 4097
        ([], [], None),                                                    # no world
        (p, v[:2], None),                                                  # lists of different lengths
        (p, v, w[:2]),
        (p, v, [a.astype(F64) for a in w]),                                # weights are integers
        (p, v, [w[0], np.ones(4, np.uint32), w[2]]),                       # a weight of the wrong length
        (p, [v[0], np.zeros((6, 2), F64), v[2]], None),                    # a velocity of another shape
        ([np.zeros((8, 3), F64)], [np.zeros((8, 3), F64)], None),          # not x,y
        (p[0], v, None),                                                   # an array where a list of worlds belongs
    ]
    for pos, vel, wgt in bad:
        with pytest.raises(ValueError):
            nb.RaggedEnsemble64(pos, vel, wgt)
    # more than 2^26 rows, without a gigabyte of zeros: broadcast views have the shape and cost nothing
    big = [np.broadcast_to(np.zeros((1, 2), F64), (4096, 2))] * ((1 << 14) + 1)
    with pytest.raises(ValueError, match="2\\^26"):
        nb.RaggedEnsemble64(big, big)
    for arith in ("double", "f64", None):
        with pytest.raises(ValueError):
            nb.RaggedEnsemble64(p, v, arith=arith)
    # each class names itself and points at its sibling
    with pytest.raises(ValueError, match="^RaggedEnsemble64: world 0: position must be float64.*RaggedEnsemble takes float32"):
        nb.RaggedEnsemble64(*_worlds([8, 5], F32))
    with pytest.raises(ValueError, match="^RaggedEnsemble: world 0: position must be float32.*RaggedEnsemble64"):
        nb.RaggedEnsemble(p, v)
    assert not made


def test_checked_ragged_takes_a_dtype_and_defaults_to_float32(nb):
    from nbody_simulation_amd.ensemble import _checked_ragged
    sizes = [3, 1, 4096, 2]
    pos = [np.full((n, 2), k + 0.5, F64) for k, n in enumerate(sizes)]
    vel = [np.full((n, 2), -k - 0.5, F64) for k, n in enumerate(sizes)]
    wgt = [np.full(n, k + 1, np.int64) for k, n in enumerate(sizes)]
    s, p, v, w = _checked_ragged(pos, vel, wgt, F64)
    assert s.dtype == np.int64 and s.tolist() == sizes
    assert p.shape == v.shape == (sum(sizes), 2) and p.dtype == v.dtype == F64 and w.dtype == np.uint32 and w.shape == (sum(sizes),)
    assert p[:, 0].tolist() == sum(([k + 0.5] * n for k, n in enumerate(sizes)), []) and np.array_equal(v, -p)
    assert _checked_ragged(pos, vel, None, F64)[3] is None
    with pytest.raises(ValueError):
        _checked_ragged(pos, vel, wgt)                                     # the default dtype is still the f32 handle's
    assert _checked_ragged(*_worlds([2, 3], F32), None)[1].dtype == F32


# ------------------------------------------------------------------ handle-free calls
@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_ragged64_has_no_cpu_fallback(nb):
    C = nb._capi
    lib = C.load()
    h = ctypes.c_void_p()
    assert lib.nbody_ragged64_create(ctypes.byref(h), 0) == C.ERR_NO_DEVICE and not h.value
    msg = lib.nbody_ragged64_last_error(None)
    assert msg and b"no CPU path" in msg and b"nbody_ragged64_create" in msg
    with pytest.raises(C.NBodyError) as e:
        nb.RaggedEnsemble64(*_worlds([2, 4]))
    assert e.value.code == C.ERR_NO_DEVICE and "no CPU path" in str(e.value)


@pytest.mark.parametrize("which", ["product", "lab"])
def test_null_handle_calls(nb, which):
    C = nb._capi
    lib = C._load(which)
    prm = C.default_params()
    buf = np.zeros(8, F64)
    w = np.ones(4, np.uint32)
    sizes = np.array([1, 3], np.int64)
    assert lib.nbody_ragged64_create(None, 0) == C.ERR_INVALID and lib.nbody_ragged64_last_error(None)
    assert lib.nbody_ragged64_set_params(None, ctypes.byref(prm)) == C.ERR_INVALID
    assert lib.nbody_ragged64_get_params(None, ctypes.byref(prm)) == C.ERR_INVALID
    assert lib.nbody_ragged64_upload(None, 2, C._ptr(sizes), C._ptr(buf), C._ptr(buf), C._ptr(w)) == C.ERR_INVALID
    assert lib.nbody_ragged64_download(None, C._ptr(buf), C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_ragged64_update(None, 0.1, 1, None) == C.ERR_INVALID
    assert lib.nbody_ragged64_update(None, 0.1, 0, None) == C.ERR_INVALID
    assert lib.nbody_ragged64_accel(None, C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_ragged64_sizes(None, C._ptr(sizes)) == C.ERR_INVALID
    assert lib.nbody_ragged64_num_worlds(None) == 0 and lib.nbody_ragged64_num_rows(None) == 0
    lib.nbody_ragged64_destroy(None)
    assert not buf.any() and sizes.tolist() == [1, 3] and w.tolist() == [1, 1, 1, 1]
    # the plan needs no handle: every output may be NULL, and bad sizes are refused with a message that names "ragged"
    assert lib.nbody_ragged64_plan(2, C._ptr(sizes), None, None, None, None, None) == C.OK
    launch = np.full(2, -7, np.int32)
    for bad in ([0, 3], [1, 4097], [-1, 3]):
        b = np.array(bad, np.int64)
        assert lib.nbody_ragged64_plan(2, C._ptr(b), C._ptr(launch), None, None, None, None) == C.ERR_INVALID
        assert b"ragged" in lib.nbody_ragged64_last_error(None)
    assert lib.nbody_ragged64_plan(0, C._ptr(sizes), C._ptr(launch), None, None, None, None) == C.ERR_INVALID
    assert lib.nbody_ragged64_plan(2, None, C._ptr(launch), None, None, None, None) == C.ERR_INVALID
    assert launch.tolist() == [-7, -7]                                     # nothing was written


@pytest.mark.parametrize("which", ["product", "lab"])
def test_the_create_error_slots_are_kept_apart(nb, which):
    C = nb._capi
    lib = C._load(which)
    assert lib.nbody_ragged_create(None, 0) == C.ERR_INVALID
    assert lib.nbody_ragged64_create(None, 0) == C.ERR_INVALID
    assert lib.nbody_ensemble64_create(None, 0) == C.ERR_INVALID
    assert lib.nbody_ragged_last_error(None).startswith(b"nbody_ragged_create:")
    assert lib.nbody_ragged64_last_error(None).startswith(b"nbody_ragged64_create:")
    assert lib.nbody_ensemble64_last_error(None).startswith(b"nbody_ensemble64_create:")
    # a refused f64 plan lands in the f64 ragged slot and leaves the other two alone
    bad = np.array([4097], np.int64)
    assert lib.nbody_ragged64_plan(1, C._ptr(bad), None, None, None, None, None) == C.ERR_INVALID
    assert lib.nbody_ragged64_last_error(None).startswith(b"ragged:")
    assert lib.nbody_ragged_last_error(None).startswith(b"nbody_ragged_create:")
    assert lib.nbody_ensemble64_last_error(None).startswith(b"nbody_ensemble64_create:")
    # ... and the other way round
    assert lib.nbody_ragged64_create(None, 0) == C.ERR_INVALID
    assert lib.nbody_ragged_plan(1, C._ptr(bad), None, None, None, None, None) == C.ERR_INVALID
    assert lib.nbody_ragged_last_error(None).startswith(b"ragged:")
    assert lib.nbody_ragged64_last_error(None).startswith(b"nbody_ragged64_create:")


def test_header_declares_the_f64_ragged_calls_and_both_libraries_export_them(nb):
    C = nb._capi
    declared = C.declared_symbols()
    assert len(NAMES) == 13 and not [s for s in NAMES if s.startswith("nbody_ragged_")]
    assert sorted(s for s in declared if s.startswith("nbody_ragged64_")) == sorted(NAMES)
    assert sorted(s for s in C._SIGS if s.startswith("nbody_ragged64_")) == sorted(NAMES)
    for path in (C.LIB_PATH, C.LAB_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in NAMES if not hasattr(lib, s)], path
    with open(C.HEADER_PATH) as f:
        assert int(re.search(r"#define\s+NBODY_ABI_VERSION\s+(\d+)", f.read()).group(1)) == 3       # new symbols only
    with open(os.path.join(os.path.dirname(C.HEADER_PATH), "nbody_ensemble.h")) as f:
        ens = f.read()
    assert "typedef struct nbody_ragged64 nbody_ragged64;" in ens
    assert ens.index("nbody_ragged_plan(") < ens.index("typedef struct nbody_ragged64")             # below the f32 ragged block
    assert "f64 ragged ensembles" not in ens                                                        # no longer "not offered"
    assert nb.RaggedEnsemble64 is nb.ensemble.RaggedEnsemble64 and nb.RaggedEnsemble64 is not nb.RaggedEnsemble
    assert not issubclass(nb.RaggedEnsemble64, nb.RaggedEnsemble) and not issubclass(nb.RaggedEnsemble, nb.RaggedEnsemble64)
    assert "RaggedEnsemble64" in nb.__all__
    assert (C.Ragged64Handle._prefix, C.Ragged64Handle._suffix, C.Ragged64Handle._dtype) == ("nbody_ragged64", "", F64)
    assert issubclass(C.Ragged64Handle, C.RaggedHandle)


# ------------------------------------------------------------------ the f64 plan
def _check_plan64(nb, monkeypatch, sizes):
    """tests/test_ragged_host.py's _check_plan, every property block by block, on the f64 plan: its LDS restatement and the plan
    it asks for are swapped for the f64 ones, nothing else."""
    monkeypatch.setattr(f32_host, "_lds", _lds64)

    class _NB64:
        @staticmethod
        def ragged_plan(s):
            return nb.ragged_plan(s, dtype=F64)

    return f32_host._check_plan(_NB64, sizes)


def test_f64_plan_covers_every_world_and_tile_exactly_once(nb, monkeypatch):
    rng = np.random.default_rng(20261019)
    sizes = PLAN_SIZES * 3 + [128, 129, 4096, 1]
    sizes = [int(n) for n in rng.permutation(sizes)]
    plan = _check_plan64(nb, monkeypatch, sizes)
    assert plan["lds_bytes"].tolist() == [2560, 5120, 10240, 20480, 40960, 81920] == [_lds64(c) for c in CAPS]
    # classes without a world launch nothing, and the LDS is that of the largest member, not of the class cap
    plan = _check_plan64(nb, monkeypatch, [300, 7, 1000, 12, 290])
    assert plan["lds_bytes"].tolist() == [_lds64(12), _lds64(300), _lds64(1000)] == [320, 6080, 20000]
    assert plan["blocks"].tolist() == [2, 4, 4]
    assert plan["launch_of_world"].tolist() == [1, 0, 2, 0, 1] and plan["first_block_of_world"].tolist() == [0, 0, 0, 1, 2]
    # either side of the 64 KiB dynamic-LDS limit
    assert _lds64(3272) == 65440 and _lds64(3273) == 65600
    assert _check_plan64(nb, monkeypatch, [3273, 2049, 4096, 3272])["lds_bytes"].tolist() == [81920]
    assert _check_plan64(nb, monkeypatch, [3272, 2049])["lds_bytes"].tolist() == [65440]
    # 10^4 worlds of random sizes
    _check_plan64(nb, monkeypatch, [int(n) for n in rng.integers(1, 4097, 10_000)])
    # classes, tiles and items are the f32 plan's: only the LDS differs
    p32 = nb.ragged_plan(sizes, dtype=F32)
    p64 = nb.ragged_plan(sizes, dtype=F64)
    for key in ("launch_of_world", "first_block_of_world", "blocks"):
        assert np.array_equal(p32[key], p64[key]), key


@pytest.mark.parametrize("n", [1, 5, 64, 128, 129, 300, 1024, 3272, 3273, 4096])
def test_f64_plan_of_equal_sizes_is_the_uniform_launch(nb, monkeypatch, n):
    for b in (1, 5):
        plan = _check_plan64(nb, monkeypatch, [n] * b)
        assert plan["lds_bytes"].tolist() == [_lds64(n)] and plan["blocks"].tolist() == [b * _tiles(n)]
        assert plan["launch_of_world"].tolist() == [0] * b
        assert plan["first_block_of_world"].tolist() == [k * _tiles(n) for k in range(b)]
    assert _lds64(1) == 160 and _lds64(8) == 160 and _lds64(9) == 320 and _lds64(4096) == 81920


def test_plan_without_a_dtype_is_unchanged(nb):
    sizes = [300, 7, 1000, 12, 290]
    plan = nb.ragged_plan(sizes)
    assert plan["lds_bytes"].tolist() == [(12 + 1) // 2 * 24, (300 + 1) // 2 * 24, (1000 + 1) // 2 * 24]
    assert plan["blocks"].tolist() == [2, 4, 4]
    again = nb.ragged_plan(sizes, dtype=F32)
    assert all(np.array_equal(plan[k], again[k]) for k in plan)
    launch, first, lds, blocks = nb._capi.ragged_plan(sizes)
    assert lds.tolist() == plan["lds_bytes"].tolist() and nb._capi.ragged_plan(sizes, f64=True)[2].tolist() == [320, 6080, 20000]
    with pytest.raises(ValueError):
        nb.ragged_plan(sizes, dtype=np.float16)


def test_f64_plan_refuses_sizes_outside_the_limits(nb):
    C = nb._capi
    for bad in ([], [0], [4097], [5, -1]):
        with pytest.raises(ValueError):
            nb.ragged_plan(bad, dtype=F64)
    with pytest.raises(C.NBodyError) as e:
        C.ragged_plan([4096] * ((1 << 14) + 1), f64=True)                  # 2^26 + 4096 rows
    assert e.value.code == C.ERR_INVALID and "ragged" in str(e.value) and "2^26" in str(e.value)
    C.ragged_plan([4096] * (1 << 14), f64=True)                            # 2^26 exactly
