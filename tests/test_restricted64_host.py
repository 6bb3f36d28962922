"""Restricted ensembles in f64 (nbody_restricted64_*, nb.RestrictedEnsemble64) without a GPU: argument checks that must fire
before any handle exists, the refusal to run without a device, NULL-handle calls, and the declared names in both libraries."""
import ctypes
import os
import re

import numpy as np
import pytest

F32, F64 = np.float32, np.float64
# fifteen, named as nbody_ensemble64_* are: no type suffix
NAMES = ["nbody_restricted64_" + s for s in ("create", "destroy", "last_error", "set_params", "get_params", "upload", "download",
                                             "tracers_upload", "tracers_download", "num_worlds", "num_bodies", "num_tracers",
                                             "update", "accel", "tracers_accel")]


def _z(*shape, dtype=F64):
    return np.zeros(shape, dtype)


def test_header_declares_the_f64_restricted_calls_and_both_libraries_export_them(nb):
    C = nb._capi
    assert len(NAMES) == 15
    declared = C.declared_symbols()
    assert sorted(s for s in declared if s.startswith("nbody_restricted64_")) == sorted(NAMES)
    assert sorted(s for s in C._SIGS if s.startswith("nbody_restricted64_")) == sorted(NAMES)
    for path in (C.LIB_PATH, C.LAB_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in NAMES if not hasattr(lib, s)], path
    with open(C.HEADER_PATH) as f:
        head = f.read()
    assert int(re.search(r"#define\s+NBODY_ABI_VERSION\s+(\d+)", head).group(1)) == 3 == C.ABI_VERSION    # new symbols only
    assert "nbody_restricted64" not in head                                 # declared in nbody_ensemble.h, which it includes
    with open(os.path.join(os.path.dirname(C.HEADER_PATH), "nbody_ensemble.h")) as f:
        text = f.read()
    assert "typedef struct nbody_restricted64 nbody_restricted64;" in text
    assert text.index("nbody_restricted_tracers_accel_f32(") < text.index("typedef struct nbody_restricted64")   # below the f32 block
    assert "RestrictedEnsemble64" in nb.__all__ and nb.RestrictedEnsemble64 is nb.ensemble.RestrictedEnsemble64
    assert not issubclass(nb.RestrictedEnsemble64, nb.RestrictedEnsemble)   # siblings
    assert not issubclass(nb.RestrictedEnsemble, nb.RestrictedEnsemble64)
    h = C.Restricted64Handle
    assert (h._prefix, h._suffix, h._dtype) == ("nbody_restricted64", "", F64)
    assert issubclass(h, C.Ensemble64Handle) and not issubclass(h, C.RestrictedHandle)
    for name in ("n_tracers", "upload_tracers", "download_tracers", "tracers_accel"):   # the tracer methods RestrictedHandle has
        assert hasattr(C.RestrictedHandle, name) and hasattr(h, name), name


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_restricted64_has_no_cpu_fallback(nb):
    C = nb._capi
    lib = C.load()
    h = ctypes.c_void_p()
    assert lib.nbody_restricted64_create(ctypes.byref(h), 0) == C.ERR_NO_DEVICE and not h.value
    msg = lib.nbody_restricted64_last_error(None)
    assert msg and msg.startswith(b"nbody_restricted64_create:") and b"no CPU path" in msg
    with pytest.raises(C.NBodyError) as e:
        nb.RestrictedEnsemble64(_z(2, 3, 2), _z(2, 3, 2), tracers=(_z(2, 5, 2), _z(2, 5, 2)))
    assert e.value.code == C.ERR_NO_DEVICE and "no CPU path" in str(e.value)


@pytest.mark.parametrize("which", ["product", "lab"])
def test_null_handle_calls(nb, which):
    C = nb._capi
    lib = C._load(which)
    prm = C.default_params()
    buf = np.zeros(8, F64)
    w = np.ones(4, np.uint32)
    assert lib.nbody_restricted64_create(None, 0) == C.ERR_INVALID
    msg = lib.nbody_restricted64_last_error(None)
    assert msg and msg.startswith(b"nbody_restricted64_create:")
    assert lib.nbody_restricted64_set_params(None, ctypes.byref(prm)) == C.ERR_INVALID
    assert lib.nbody_restricted64_get_params(None, ctypes.byref(prm)) == C.ERR_INVALID
    assert lib.nbody_restricted64_upload(None, 1, 4, C._ptr(buf), C._ptr(buf), C._ptr(w)) == C.ERR_INVALID
    assert lib.nbody_restricted64_download(None, C._ptr(buf), C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_restricted64_tracers_upload(None, 1, 4, C._ptr(buf), C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_restricted64_tracers_download(None, C._ptr(buf), C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_restricted64_update(None, 0.1, 1, None) == C.ERR_INVALID
    assert lib.nbody_restricted64_accel(None, C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_restricted64_tracers_accel(None, C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_restricted64_num_worlds(None) == 0 and lib.nbody_restricted64_num_bodies(None) == 0
    assert lib.nbody_restricted64_num_tracers(None) == 0
    lib.nbody_restricted64_destroy(None)
    assert not buf.any() and w.tolist() == [1, 1, 1, 1]


@pytest.mark.parametrize("which", ["product", "lab"])
def test_the_three_create_errors_are_kept_apart(nb, which):
    """nbody_restricted_*, nbody_restricted64_* and nbody_ensemble64_* each keep the message of their own last failed create:
    whichever of the three fails afterwards, the other two slots keep their bytes."""
    C = nb._capi
    lib = C._load(which)
    creates = {p: getattr(lib, p + "_create") for p in ("nbody_restricted", "nbody_restricted64", "nbody_ensemble64")}
    errors = {p: getattr(lib, p + "_last_error") for p in creates}
    for p, create in creates.items():
        assert create(None, 0) == C.ERR_INVALID
    first = {p: errors[p](None) for p in creates}
    for p, msg in first.items():
        assert msg and msg.startswith(p.encode() + b"_create:"), (p, msg)
    assert len(set(first.values())) == 3
    for p, create in creates.items():           # one at a time, another kind of failure: its own slot changes, the others do not
        h = ctypes.c_void_p()
        rc = create(ctypes.byref(h), -1)
        assert rc != C.OK and not h.value
        now = {q: errors[q](None) for q in creates}
        assert now[p].startswith(p.encode() + b"_create:")
        for q in creates:
            if q != p:
                assert now[q] == first[q], (p, q)
        first = now


def test_restricted64_rejects_bad_input_before_any_handle_exists(nb, monkeypatch):
    C = nb._capi
    made = []
    monkeypatch.setattr(C, "Restricted64Handle", lambda *a, **k: made.append(1) or pytest.fail("a handle was created"))
    p, v = _z(3, 8, 2), _z(3, 8, 2)
    tr = (_z(3, 5, 2), _z(3, 5, 2))
    bad = [
        dict(position=p.astype(F32), velocity=v.astype(F32)),                               # wrong dtype
        dict(position=p, velocity=v.astype(F32)),
        dict(position=p, velocity=v, tracers=(tr[0].astype(F32), tr[1])),
        dict(position=p, velocity=v, tracers=(tr[0], tr[1].astype(F32))),
        dict(position=_z(3, 8, 3), velocity=_z(3, 8, 3)),                                   # position not [B, n, 2]
        dict(position=_z(3, 8), velocity=_z(3, 8)),
        dict(position=p, velocity=_z(3, 7, 2)),                                             # a velocity of another shape
        dict(position=p, velocity=v, tracers=tr[0]),                                        # tracers not a pair
        dict(position=p, velocity=v, tracers=(tr[0],)),
        dict(position=p, velocity=v, tracers=(_z(3, 5, 3), _z(3, 5, 3))),                   # ... of [B, m, 2]
        dict(position=p, velocity=v, tracers=(_z(5, 2), _z(5, 2))),                         # ([m, 2] is for one world only)
        dict(position=p, velocity=v, tracers=(tr[0], _z(3, 6, 2))),                         # a tracer velocity of another shape
        dict(position=p, velocity=v, tracers=(_z(2, 5, 2), _z(2, 5, 2))),                   # tracer B != body B
        dict(position=_z(3, 0, 2), velocity=_z(3, 0, 2)),                                   # n = 0
        dict(position=_z(1, 4097, 2), velocity=_z(1, 4097, 2)),                             # n = 4097
        dict(position=p, velocity=v, weight=np.ones((3, 8), F64)),                          # weights are integers
    ]
    for kw in bad:
        with pytest.raises(ValueError, match="RestrictedEnsemble64"):
            nb.RestrictedEnsemble64(**kw)
    # B * m > 2^26 without a gigabyte of zeros: zero-stride views have the shape and cost nothing
    big = np.broadcast_to(np.zeros((1, 1, 2), F64), (3, (1 << 26) // 3 + 1, 2))
    with pytest.raises(ValueError, match=r"RestrictedEnsemble64.*tracers.*2\^26"):
        nb.RestrictedEnsemble64(p, v, tracers=(big, big))
    bodies = np.broadcast_to(np.zeros((1, 1, 2), F64), ((1 << 14) + 1, 4096, 2))
    with pytest.raises(ValueError, match=r"RestrictedEnsemble64.*2\^26"):
        nb.RestrictedEnsemble64(bodies, bodies)
    with pytest.raises(ValueError):
        nb.RestrictedEnsemble64(p, v, tracers=tr, arith="double")
    assert not made


def test_checked_tracers_takes_a_dtype_and_keeps_its_float32_default(nb):
    from nbody_simulation_amd.ensemble import _checked_tracers
    assert _checked_tracers(None, 4, "RestrictedEnsemble64", F64) == (0, None, None)
    m, tp, tv = _checked_tracers((np.ones((2, 7, 2))[:, ::2], np.ones((2, 4, 2))), 2, "RestrictedEnsemble64", F64)
    assert m == 4 and tp.flags.c_contiguous and tp.shape == tv.shape == (2, 4, 2) and tp.dtype == tv.dtype == F64
    m, tp, tv = _checked_tracers((_z(5, 2), _z(5, 2)), 1, dtype=F64)     # one world: [m, 2]
    assert m == 5 and tp.shape == tv.shape == (1, 5, 2)
    m, tp, tv = _checked_tracers((_z(2, 0, 2), _z(2, 0, 2)), 2, dtype=F64)   # m = 0 removes them
    assert m == 0
    # the default is float32, under RestrictedEnsemble's name and with its message
    m, tp, tv = _checked_tracers((_z(2, 3, 2, dtype=F32), _z(2, 3, 2, dtype=F32)), 2)
    assert m == 3 and tp.dtype == F32
    with pytest.raises(ValueError, match=r"^RestrictedEnsemble: tracer position must be float32 \(got float64\)$"):
        _checked_tracers((_z(2, 3, 2), _z(2, 3, 2)), 2)
    with pytest.raises(ValueError, match=r"^RestrictedEnsemble64: tracer velocity must be float64 \(got float32\)"):
        _checked_tracers((_z(2, 3, 2), _z(2, 3, 2, dtype=F32)), 2, "RestrictedEnsemble64", F64)
