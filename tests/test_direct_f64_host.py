"""CPU-side checks of the f64 direct entry points (nbody_update_direct_f64, nbody_accel_direct_f64): both libraries export
them, and they refuse a NULL context before touching any device.  No GPU."""
import ctypes

import pytest

SYMBOLS = ("nbody_update_direct_f64", "nbody_accel_direct_f64")


@pytest.mark.parametrize("which", ["product", "lab"])
def test_f64_direct_symbols_are_exported(nb, which):
    C = nb._capi
    lib = ctypes.CDLL(C.LIB_PATH if which == "product" else C.LAB_LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(C.declared_symbols())


@pytest.mark.parametrize("which", ["product", "lab"])
def test_f64_direct_calls_refuse_a_null_context(nb, which):
    C = nb._capi
    lib = ctypes.CDLL(C.LIB_PATH if which == "product" else C.LAB_LIB_PATH)
    upd = lib.nbody_update_direct_f64
    upd.restype, upd.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_void_p]
    acc = lib.nbody_accel_direct_f64
    acc.restype, acc.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]
    out = (ctypes.c_double * 2)()
    assert upd(None, 0.1, 1, None) == C.ERR_INVALID
    assert acc(None, out) == C.ERR_INVALID


def test_abi_version_names_the_f64_direct_calls(nb):
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbody_hip.h")) as f:
        hdr = f.read()
    assert nb._capi.ABI_VERSION == 3
    assert "3: nbody_update_direct_f64, nbody_accel_direct_f64" in hdr
