"""Ensembles in f64 (nbody_ensemble64_*, nb.Ensemble64) without a GPU: argument checks that must fire before any handle exists,
the refusal to run without a device, NULL-handle calls, and the declared names in both libraries."""
import ctypes
import os
import re

import numpy as np
import pytest

F32, F64 = np.float32, np.float64
NAMES = ["nbody_ensemble64_" + s for s in ("create", "destroy", "last_error", "set_params", "get_params", "upload", "download",
                                           "num_worlds", "num_bodies", "update", "accel")]


def _world(b, n, dtype=F64):
    return np.zeros((b, n, 2), dtype), np.zeros((b, n, 2), dtype)


def test_ensemble64_rejects_bad_input_before_any_handle_exists(nb, monkeypatch):
    C = nb._capi
    made = []
    monkeypatch.setattr(C, "Ensemble64Handle", lambda *a, **k: made.append(1) or pytest.fail("a handle was created"))
    monkeypatch.setattr(C, "EnsembleHandle", lambda *a, **k: made.append(1) or pytest.fail("an f32 handle was created"))
    p, v = _world(3, 8)
    bad = [
        (p.astype(F32), v.astype(F32), None),                              # float32: that is nb.Ensemble's
        (p, v.astype(F32), None),                                          # mixed dtypes
        (p.astype(F32), v, None),
        (np.zeros((3, 8, 3), F64), np.zeros((3, 8, 3), F64), None),        # not x,y
        (np.zeros((3, 8), F64), np.zeros((3, 8), F64), None),              # a 2-D array whose rows are not x,y
        (np.zeros((2, 3, 8, 2), F64), np.zeros((2, 3, 8, 2), F64), None),  # too many axes
        (p, np.zeros((3, 7, 2), F64), None),                               # velocity of another shape
        (*_world(2, 0), None),                                             # n = 0
        (*_world(1, 4097), None),                                          # n = 4097
        (*_world(0, 8), None),                                             # no world
        (p, v, np.ones((3, 7), np.uint32)),                                # weight of the wrong shape
        (p, v, np.ones(24, np.uint32)),
        (p, v, np.ones((3, 8), F64)),                                      # weights are integers
        (p, v, np.ones((3, 8), F32)),
    ]
    for pos, vel, w in bad:
        with pytest.raises(ValueError):
            nb.Ensemble64(pos, vel, w)
    # B * n > 2^26, without a gigabyte of zeros: a broadcast view has the shape and costs nothing
    big = np.broadcast_to(np.zeros((1, 1, 2), F64), ((1 << 14) + 1, 4096, 2))
    with pytest.raises(ValueError, match="2\\^26"):
        nb.Ensemble64(big, big)
    for arith in ("double", "f64", None):
        with pytest.raises(ValueError):
            nb.Ensemble64(p, v, arith=arith)
    with pytest.raises(ValueError, match="^Ensemble64: position must be float64"):   # the message names the class in hand
        nb.Ensemble64(p.astype(F32), v.astype(F32))
    # and the f32 ensemble goes on refusing float64, now pointing at this one
    with pytest.raises(ValueError, match="Ensemble64"):
        nb.Ensemble(p, v)
    assert not made


def test_checked_shapes_that_are_fine(nb):
    from nbody_simulation_amd.ensemble import _checked
    p, v = _world(3, 8)
    b, n, pp, vv, w = _checked(p, v, None, F64)
    assert (b, n, pp.dtype, vv.dtype, w) == (3, 8, F64, F64, None)
    b, n, pp, vv, w = _checked(p[0], v[0], np.arange(8), F64)               # 2-D position: one world
    assert (b, n, pp.shape, vv.shape, w.shape, w.dtype) == (1, 8, (1, 8, 2), (1, 8, 2), (1, 8), np.uint32)
    assert _checked(*_world(1, 4096), None, F64)[:2] == (1, 4096)
    assert _checked(*_world(1, 1), None, F64)[:2] == (1, 1)
    assert _checked(*_world(3, 8, F32), None)[:2] == (3, 8)                 # the default dtype is still the f32 ensemble's


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_ensemble64_has_no_cpu_fallback(nb):
    C = nb._capi
    lib = C.load()
    h = ctypes.c_void_p()
    assert lib.nbody_ensemble64_create(ctypes.byref(h), 0) == C.ERR_NO_DEVICE and not h.value
    msg = lib.nbody_ensemble64_last_error(None)
    assert msg and b"no CPU path" in msg
    with pytest.raises(C.NBodyError) as e:
        nb.Ensemble64(*_world(2, 4))
    assert e.value.code == C.ERR_NO_DEVICE and "no CPU path" in str(e.value)


@pytest.mark.parametrize("which", ["product", "lab"])
def test_null_handle_calls(nb, which):
    C = nb._capi
    lib = C._load(which)
    prm = C.default_params()
    buf = np.zeros(8, F64)
    w = np.ones(4, np.uint32)
    assert lib.nbody_ensemble64_create(None, 0) == C.ERR_INVALID and lib.nbody_ensemble64_last_error(None)
    assert lib.nbody_ensemble64_set_params(None, ctypes.byref(prm)) == C.ERR_INVALID
    assert lib.nbody_ensemble64_get_params(None, ctypes.byref(prm)) == C.ERR_INVALID
    assert lib.nbody_ensemble64_upload(None, 1, 4, C._ptr(buf), C._ptr(buf), C._ptr(w)) == C.ERR_INVALID
    assert lib.nbody_ensemble64_download(None, C._ptr(buf), C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_ensemble64_update(None, 0.1, 1, None) == C.ERR_INVALID
    assert lib.nbody_ensemble64_update(None, 0.1, 0, None) == C.ERR_INVALID
    assert lib.nbody_ensemble64_accel(None, C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_ensemble64_num_worlds(None) == 0 and lib.nbody_ensemble64_num_bodies(None) == 0
    lib.nbody_ensemble64_destroy(None)
    assert not buf.any() and w.tolist() == [1, 1, 1, 1]


@pytest.mark.parametrize("which", ["product", "lab"])
def test_the_two_create_errors_are_kept_apart(nb, which):
    C = nb._capi
    lib = C._load(which)
    assert lib.nbody_ensemble_create(None, 0) == C.ERR_INVALID
    assert lib.nbody_ensemble64_create(None, 0) == C.ERR_INVALID
    assert lib.nbody_ensemble_last_error(None).startswith(b"nbody_ensemble_create:")
    assert lib.nbody_ensemble64_last_error(None).startswith(b"nbody_ensemble64_create:")


def test_header_declares_the_f64_ensemble_and_both_libraries_export_it(nb):
    C = nb._capi
    declared = C.declared_symbols()
    assert sorted(s for s in declared if s.startswith("nbody_ensemble64_")) == sorted(NAMES)
    assert set(NAMES) <= set(C._SIGS)
    for path in (C.LIB_PATH, C.LAB_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in NAMES if not hasattr(lib, s)], path
    with open(os.path.join(os.path.dirname(C.HEADER_PATH), "nbody_ensemble.h")) as f:
        text = f.read()
    assert "typedef struct nbody_ensemble64 nbody_ensemble64;" in text
    assert text.index("nbody_ensemble_accel_f32(") < text.index("typedef struct nbody_ensemble64")   # below the f32 block
    with open(C.HEADER_PATH) as f:
        assert int(re.search(r"#define\s+NBODY_ABI_VERSION\s+(\d+)", f.read()).group(1)) == 3       # new symbols only
    assert nb.Ensemble64 is nb.ensemble.Ensemble64 and nb.Ensemble64 is not nb.Ensemble
    assert not issubclass(nb.Ensemble64, nb.Ensemble) and not issubclass(nb.Ensemble, nb.Ensemble64)   # siblings
    assert C.Ensemble64Handle is not C.EnsembleHandle
