"""CPU-side checks of the direct sum at arbitrary points (nbody_accel_direct_at_f32 / _f64): both libraries export the two
symbols, the header declares them, the binding binds them, a NULL context is refused before any device is touched, and the
Rust block of INTEGRATION.md names them.  No GPU."""
import ctypes
import os

import pytest

SYMBOLS = ("nbody_accel_direct_at_f32", "nbody_accel_direct_at_f64")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("which", ["product", "lab"])
def test_probe_symbols_are_exported_and_declared(nb, which):
    C = nb._capi
    lib = ctypes.CDLL(C.LIB_PATH if which == "product" else C.LAB_LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    assert set(SYMBOLS) <= set(C.declared_symbols())


def test_the_binding_binds_them(nb):
    C = nb._capi
    lib = C.load()
    for s in SYMBOLS:
        assert s in C._SIGS
        assert getattr(lib, s).restype is ctypes.c_int
    assert "targets" in C.Context.accel_direct.__code__.co_varnames
    assert C.MultiContext.accel_direct is C.Context.accel_direct


@pytest.mark.parametrize("which", ["product", "lab"])
def test_probe_calls_refuse_a_null_context(nb, which):
    C = nb._capi
    lib = ctypes.CDLL(C.LIB_PATH if which == "product" else C.LAB_LIB_PATH)
    tgt32, acc32 = (ctypes.c_float * 2)(1.0, 2.0), (ctypes.c_float * 2)()
    tgt64, acc64 = (ctypes.c_double * 2)(1.0, 2.0), (ctypes.c_double * 2)()
    f32, f64 = lib.nbody_accel_direct_at_f32, lib.nbody_accel_direct_at_f64
    for f in (f32, f64):
        f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    assert f32(None, 1, tgt32, acc32) == C.ERR_INVALID
    assert f64(None, 1, tgt64, acc64) == C.ERR_INVALID
    assert f32(None, 0, None, None) == C.ERR_INVALID
    assert tuple(acc32) == (0.0, 0.0) and tuple(acc64) == (0.0, 0.0)


def test_integration_rust_block_names_them():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        md = f.read()
    for s in SYMBOLS:
        assert f"pub fn {s}(ctx: *mut NbodyCtx, n_targets: i64," in md, s


def test_abi_version_stays_3_and_says_the_calls_were_added(nb):
    with open(os.path.join(ROOT, "include", "nbody_hip.h")) as f:
        hdr = f.read()
    assert nb._capi.ABI_VERSION == 3
    assert "nbody_accel_direct_at_f32 / _f64 (the direct sum at arbitrary points) were added under 3" in hdr
