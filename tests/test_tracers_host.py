"""CPU-side checks of the tracers (nbody_tracers_upload_f32 / _f64, nbody_tracers_download_f32 / _f64, nbody_num_tracers): the
header declares the five names, both libraries export them, the binding binds them, a NULL context is refused before any device
is touched, and scenes.restricted splits the reference's scene into its two heavy bodies and the rest.  No GPU."""
import ctypes

import numpy as np
import pytest

SYMBOLS = ("nbody_tracers_upload_f32", "nbody_tracers_upload_f64", "nbody_tracers_download_f32", "nbody_tracers_download_f64",
           "nbody_num_tracers")


@pytest.mark.parametrize("which", ["product", "lab"])
def test_tracer_symbols_are_declared_exported_and_bound(nb, which):
    C = nb._capi
    lib = ctypes.CDLL(C.LIB_PATH if which == "product" else C.LAB_LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
        assert s in C._SIGS, s
    assert set(SYMBOLS) <= set(C.declared_symbols())
    assert set(C._SIGS) == set(C.declared_symbols())
    assert C._SIGS["nbody_num_tracers"][0] is ctypes.c_int64


@pytest.mark.parametrize("which", ["product", "lab"])
def test_tracer_calls_refuse_a_null_context(nb, which):
    C = nb._capi
    lib = ctypes.CDLL(C.LIB_PATH if which == "product" else C.LAB_LIB_PATH)
    for s in SYMBOLS:
        f = getattr(lib, s)
        f.restype, f.argtypes = C._SIGS[s]
    lib.nbody_last_error.restype, lib.nbody_last_error.argtypes = ctypes.c_char_p, [ctypes.c_void_p]
    assert lib.nbody_num_tracers(None) == 0
    p32, p64 = np.ones((1, 2), np.float32), np.ones((1, 2), np.float64)
    for f, a in ((lib.nbody_tracers_upload_f32, p32), (lib.nbody_tracers_upload_f64, p64)):
        assert f(None, 1, C._ptr(a), C._ptr(a)) == C.ERR_INVALID
        assert b"tracers" in lib.nbody_last_error(None)
        assert f(None, 0, None, None) == C.ERR_INVALID
    for f, a in ((lib.nbody_tracers_download_f32, p32), (lib.nbody_tracers_download_f64, p64)):
        assert f(None, C._ptr(a), C._ptr(a)) == C.ERR_INVALID
        assert b"tracers" in lib.nbody_last_error(None)
    assert np.all(p32 == 1) and np.all(p64 == 1)


def test_the_python_layers_offer_them(nb):
    C = nb._capi
    for name in ("upload_tracers", "download_tracers", "n_tracers"):
        assert hasattr(C.Context, name), name
    assert C.MultiContext.upload_tracers is not C.Context.upload_tracers
    assert "tracers" in nb.World.__init__.__code__.co_varnames and hasattr(nb.World, "tracers")


def test_restricted_splits_the_reference_scene_into_two_bodies_and_the_rest(nb):
    pos, vel, w = nb.scenes.galaxy()
    (bp, bv, bw), (tp, tv) = nb.scenes.restricted(pos, vel, w, 2)
    assert len(bp) == 2 and list(bw) == [75_000_000, 750_000] and bw.dtype == np.uint32
    assert len(tp) == len(pos) - 2 > 150_000 and tp.shape == tv.shape
    assert np.array_equal(np.concatenate([bp, tp]), pos) and np.array_equal(np.concatenate([bv, tv]), vel)
    (bp, _, bw), (tp, _) = nb.scenes.restricted(pos, vel, w, 1)
    assert len(bp) == len(pos) and tp.shape == (0, 2)
