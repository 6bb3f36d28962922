"""Ensembles (nbody_ensemble_*, nb.Ensemble) without a GPU: argument checks that must fire before any handle exists, the
refusal to run without a device, NULL-handle calls, and the declared names in both libraries."""
import ctypes
import os

import numpy as np
import pytest

F32 = np.float32


def _world(b, n, dtype=F32):
    return np.zeros((b, n, 2), dtype), np.zeros((b, n, 2), dtype)


def test_ensemble_rejects_bad_input_before_any_handle_exists(nb, monkeypatch):
    C = nb._capi
    made = []
    monkeypatch.setattr(C, "EnsembleHandle", lambda *a, **k: made.append(1) or pytest.fail("a handle was created"))
    p, v = _world(3, 8)
    bad = [
        (np.zeros((3, 8, 3), F32), np.zeros((3, 8, 3), F32), None),        # not x,y
        (np.zeros((3, 8), F32), np.zeros((3, 8), F32), None),              # a 2-D array whose rows are not x,y
        (np.zeros((2, 3, 8, 2), F32), np.zeros((2, 3, 8, 2), F32), None),  # too many axes
        (p, np.zeros((3, 7, 2), F32), None),                               # velocity of another shape
        (p.astype(np.float64), v.astype(np.float64), None),                # float64
        (p, v.astype(np.float64), None),
        (*_world(2, 0), None),                                             # n = 0
        (*_world(1, 4097), None),                                          # n = 4097
        (*_world(0, 8), None),                                             # no world
        (p, v, np.ones((3, 7), np.uint32)),                                # weight of the wrong shape
        (p, v, np.ones(24, np.uint32)),
        (p, v, np.ones((3, 8), F32)),                                      # weights are integers
    ]
    for pos, vel, w in bad:
        with pytest.raises(ValueError):
            nb.Ensemble(pos, vel, w)
    # B * n > 2^26, without 512 MB of zeros: a broadcast view has the shape and costs nothing
    big = np.broadcast_to(np.zeros((1, 1, 2), F32), ((1 << 14) + 1, 4096, 2))
    with pytest.raises(ValueError, match="2\\^26"):
        nb.Ensemble(big, big)
    with pytest.raises(ValueError):
        nb.Ensemble(p, v, arith="double")
    assert not made


def test_checked_shapes_that_are_fine(nb):
    from nbody_simulation_amd.ensemble import _checked
    p, v = _world(3, 8)
    assert _checked(p, v, None)[:2] == (3, 8)
    b, n, pp, vv, w = _checked(p[0], v[0], np.arange(8))                    # 2-D position: one world
    assert (b, n, pp.shape, vv.shape, w.shape, w.dtype) == (1, 8, (1, 8, 2), (1, 8, 2), (1, 8), np.uint32)
    assert _checked(*_world(1, 4096), None)[:2] == (1, 4096)
    assert _checked(*_world(1, 1), None)[:2] == (1, 1)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_ensemble_has_no_cpu_fallback(nb):
    C = nb._capi
    lib = C.load()
    h = ctypes.c_void_p()
    assert lib.nbody_ensemble_create(ctypes.byref(h), 0) == C.ERR_NO_DEVICE and not h.value
    msg = lib.nbody_ensemble_last_error(None)
    assert msg and b"no CPU path" in msg
    with pytest.raises(C.NBodyError) as e:
        nb.Ensemble(*_world(2, 4))
    assert e.value.code == C.ERR_NO_DEVICE and "no CPU path" in str(e.value)


@pytest.mark.parametrize("which", ["product", "lab"])
def test_null_handle_calls(nb, which):
    C = nb._capi
    lib = C._load(which)
    prm = C.default_params()
    buf = np.zeros(8, F32)
    w = np.ones(4, np.uint32)
    assert lib.nbody_ensemble_create(None, 0) == C.ERR_INVALID and lib.nbody_ensemble_last_error(None)
    assert lib.nbody_ensemble_set_params(None, ctypes.byref(prm)) == C.ERR_INVALID
    assert lib.nbody_ensemble_get_params(None, ctypes.byref(prm)) == C.ERR_INVALID
    assert lib.nbody_ensemble_upload_f32(None, 1, 4, C._ptr(buf), C._ptr(buf), C._ptr(w)) == C.ERR_INVALID
    assert lib.nbody_ensemble_download_f32(None, C._ptr(buf), C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_ensemble_update_f32(None, 0.1, 1, None) == C.ERR_INVALID
    assert lib.nbody_ensemble_accel_f32(None, C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_ensemble_num_worlds(None) == 0 and lib.nbody_ensemble_num_bodies(None) == 0
    lib.nbody_ensemble_destroy(None)
    assert not buf.any()


def test_header_declares_the_ensemble_and_both_libraries_export_it(nb):
    C = nb._capi
    names = ["nbody_ensemble_" + s for s in ("create", "destroy", "last_error", "set_params", "get_params", "upload_f32",
                                             "download_f32", "num_worlds", "num_bodies", "update_f32", "accel_f32")]
    declared = C.declared_symbols()
    assert set(names) <= set(declared) and set(names) <= set(C._SIGS)
    assert sorted(s for s in declared if s.startswith("nbody_ensemble_")) == sorted(names)
    for path in (C.LIB_PATH, C.LAB_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in names if not hasattr(lib, s)], path
    with open(C.HEADER_PATH) as f:
        head = f.read()
    assert '#include "nbody_ensemble.h"' in head            # nbody_hip.h declares them through the header it includes
    with open(os.path.join(os.path.dirname(C.HEADER_PATH), "nbody_ensemble.h")) as f:
        assert "typedef struct nbody_ensemble nbody_ensemble;" in f.read()
    import re
    assert int(re.search(r"#define\s+NBODY_ABI_VERSION\s+(\d+)", head).group(1)) == 3    # new symbols only
    assert nb.Ensemble is nb.ensemble.Ensemble
