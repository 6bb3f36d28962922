"""CPU-side checks of the tracers' hand-off calls (nbody_render_rgba_tracers, nbody_snapshot_num_tracers, nbody_snapshot_tracers_f32 /
_f64, nbody_tracers_delta_begin / _pending / _end / _reset): the header declares them, both libraries export them, the binding
binds them, the ABI version stands, and a NULL context is refused before any device is touched.  No GPU."""
import ctypes

import numpy as np
import pytest

SYMBOLS = ("nbody_render_rgba_tracers", "nbody_snapshot_num_tracers", "nbody_snapshot_tracers_f32", "nbody_snapshot_tracers_f64",
           "nbody_tracers_delta_begin", "nbody_tracers_delta_pending", "nbody_tracers_delta_end", "nbody_tracers_delta_reset")


def _bound(C, which):
    lib = ctypes.CDLL(C.LIB_PATH if which == "product" else C.LAB_LIB_PATH)
    for s in SYMBOLS + ("nbody_last_error", "nbody_abi_version"):
        f = getattr(lib, s)
        f.restype, f.argtypes = C._SIGS[s]
    return lib


@pytest.mark.parametrize("which", ["product", "lab"])
def test_handoff_symbols_are_declared_exported_and_bound(nb, which):
    C = nb._capi
    lib = ctypes.CDLL(C.LIB_PATH if which == "product" else C.LAB_LIB_PATH)
    declared = C.declared_symbols()
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in C._SIGS, s
    assert not [s for s in declared if not hasattr(lib, s)]
    assert sorted(C._SIGS) == declared
    assert C._SIGS["nbody_snapshot_num_tracers"][0] is ctypes.c_int64


@pytest.mark.parametrize("which", ["product", "lab"])
def test_abi_version_stays_3(nb, which):
    C = nb._capi
    assert _bound(C, which).nbody_abi_version() == 3 == C.ABI_VERSION
    with open(C.HEADER_PATH) as f:
        assert "#define NBODY_ABI_VERSION 3\n" in f.read()


@pytest.mark.parametrize("which", ["product", "lab"])
def test_handoff_calls_refuse_a_null_context(nb, which):
    C = nb._capi
    lib = _bound(C, which)
    rgba = np.full((10, 10, 4), 7, np.uint8)
    assert lib.nbody_render_rgba_tracers(None, 100, 10, C._ptr(rgba)) == C.ERR_INVALID
    assert b"tracers" in lib.nbody_last_error(None)
    assert lib.nbody_snapshot_num_tracers(None) == C.ERR_INVALID
    p32, p64 = np.ones((1, 2), np.float32), np.ones((1, 2), np.float64)
    assert lib.nbody_snapshot_tracers_f32(None, C._ptr(p32), C._ptr(p32)) == C.ERR_INVALID
    assert lib.nbody_snapshot_tracers_f64(None, C._ptr(p64), C._ptr(p64)) == C.ERR_INVALID
    assert lib.nbody_snapshot_tracers_f32(None, None, None) == C.ERR_INVALID
    assert lib.nbody_tracers_delta_begin(None) == C.ERR_INVALID
    assert lib.nbody_tracers_delta_pending(None) == C.ERR_INVALID
    out = np.full(64, 7, np.uint8)
    size, step = ctypes.c_size_t(11), ctypes.c_uint64(13)
    assert lib.nbody_tracers_delta_end(None, C._ptr(out), 64, ctypes.byref(size), ctypes.byref(step)) == C.ERR_INVALID
    assert lib.nbody_tracers_delta_end(None, None, 0, None, None) == C.ERR_INVALID
    assert lib.nbody_tracers_delta_reset(None) == C.ERR_INVALID
    assert b"tracers" in lib.nbody_last_error(None)
    assert np.all(rgba == 7) and np.all(out == 7) and np.all(p32 == 1) and np.all(p64 == 1)
    assert (size.value, step.value) == (11, 13)


def test_the_python_layers_offer_them(nb):
    import inspect
    C = nb._capi
    for name in ("snapshot_tracers", "tracers_delta_begin", "tracers_delta_pending", "tracers_delta_end", "tracers_delta_reset"):
        assert hasattr(C.Context, name), name
    for name in ("snapshot_tracers", "tracers_delta_begin", "tracers_delta_end"):
        assert hasattr(nb.World, name), name
    for f in (C.Context.render, nb.World.frame, nb.World.save_frame):
        assert inspect.signature(f).parameters["tracers"].default is False     # the defaults keep today's results
    assert inspect.signature(C.Context.tracers_delta_end).parameters["cap"].default is None
