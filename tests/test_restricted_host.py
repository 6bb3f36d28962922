"""Restricted ensembles (nbody_restricted_*, nb.RestrictedEnsemble) without a GPU: argument checks that must fire before any
handle exists, the refusal to run without a device, NULL-handle calls, and the declared names in both libraries."""
import ctypes
import os
import re

import numpy as np
import pytest

F32 = np.float32
# fifteen: tracers_accel_f32 is kept (FAST accelerations at the tracers without a step)
NAMES = ["nbody_restricted_" + s for s in ("create", "destroy", "last_error", "set_params", "get_params", "upload_f32", "download_f32",
                                           "tracers_upload_f32", "tracers_download_f32", "num_worlds", "num_bodies", "num_tracers",
                                           "update_f32", "accel_f32", "tracers_accel_f32")]


def _z(*shape, dtype=F32):
    return np.zeros(shape, dtype)


def test_header_declares_the_restricted_calls_and_both_libraries_export_them(nb):
    C = nb._capi
    assert len(NAMES) == 15
    declared = C.declared_symbols()
    assert sorted(s for s in declared if s.startswith("nbody_restricted_")) == sorted(NAMES)
    assert sorted(s for s in C._SIGS if s.startswith("nbody_restricted_")) == sorted(NAMES)
    for path in (C.LIB_PATH, C.LAB_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in NAMES if not hasattr(lib, s)], path
    with open(C.HEADER_PATH) as f:
        head = f.read()
    assert int(re.search(r"#define\s+NBODY_ABI_VERSION\s+(\d+)", head).group(1)) == 3 == C.ABI_VERSION    # new symbols only
    assert "nbody_restricted" not in head                                   # declared in nbody_ensemble.h, which it includes
    with open(os.path.join(os.path.dirname(C.HEADER_PATH), "nbody_ensemble.h")) as f:
        assert "typedef struct nbody_restricted nbody_restricted;" in f.read()
    assert "RestrictedEnsemble" in nb.__all__ and nb.RestrictedEnsemble is nb.ensemble.RestrictedEnsemble
    assert C.RestrictedHandle._prefix == "nbody_restricted"


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_restricted_has_no_cpu_fallback(nb):
    C = nb._capi
    lib = C.load()
    h = ctypes.c_void_p()
    assert lib.nbody_restricted_create(ctypes.byref(h), 0) == C.ERR_NO_DEVICE and not h.value
    msg = lib.nbody_restricted_last_error(None)
    assert msg and msg.startswith(b"nbody_restricted_create:") and b"no CPU path" in msg
    with pytest.raises(C.NBodyError) as e:
        nb.RestrictedEnsemble(_z(2, 3, 2), _z(2, 3, 2), tracers=(_z(2, 5, 2), _z(2, 5, 2)))
    assert e.value.code == C.ERR_NO_DEVICE and "no CPU path" in str(e.value)


@pytest.mark.parametrize("which", ["product", "lab"])
def test_null_handle_calls(nb, which):
    C = nb._capi
    lib = C._load(which)
    prm = C.default_params()
    buf = np.zeros(8, F32)
    w = np.ones(4, np.uint32)
    assert lib.nbody_restricted_create(None, 0) == C.ERR_INVALID
    msg = lib.nbody_restricted_last_error(None)
    assert msg and msg.startswith(b"nbody_restricted_create:")
    # a slot of its own: the ensemble's and the ragged ensemble's failed creates leave it alone
    assert lib.nbody_ensemble_create(None, 0) == C.ERR_INVALID and lib.nbody_ragged_create(None, 0) == C.ERR_INVALID
    assert lib.nbody_restricted_last_error(None) == msg and lib.nbody_ensemble_last_error(None) != msg
    assert lib.nbody_restricted_set_params(None, ctypes.byref(prm)) == C.ERR_INVALID
    assert lib.nbody_restricted_get_params(None, ctypes.byref(prm)) == C.ERR_INVALID
    assert lib.nbody_restricted_upload_f32(None, 1, 4, C._ptr(buf), C._ptr(buf), C._ptr(w)) == C.ERR_INVALID
    assert lib.nbody_restricted_download_f32(None, C._ptr(buf), C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_restricted_tracers_upload_f32(None, 1, 4, C._ptr(buf), C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_restricted_tracers_download_f32(None, C._ptr(buf), C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_restricted_update_f32(None, 0.1, 1, None) == C.ERR_INVALID
    assert lib.nbody_restricted_accel_f32(None, C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_restricted_tracers_accel_f32(None, C._ptr(buf)) == C.ERR_INVALID
    assert lib.nbody_restricted_num_worlds(None) == 0 and lib.nbody_restricted_num_bodies(None) == 0
    assert lib.nbody_restricted_num_tracers(None) == 0
    lib.nbody_restricted_destroy(None)
    assert not buf.any()


def test_restricted_rejects_bad_input_before_any_handle_exists(nb, monkeypatch):
    C = nb._capi
    made = []
    monkeypatch.setattr(C, "RestrictedHandle", lambda *a, **k: made.append(1) or pytest.fail("a handle was created"))
    p, v = _z(3, 8, 2), _z(3, 8, 2)
    tr = (_z(3, 5, 2), _z(3, 5, 2))
    bad = [
        dict(position=p.astype(np.float64), velocity=v.astype(np.float64)),                 # wrong dtype
        dict(position=p, velocity=v.astype(np.float64)),
        dict(position=p, velocity=v, tracers=(tr[0].astype(np.float64), tr[1])),
        dict(position=p, velocity=v, tracers=(tr[0], tr[1].astype(np.float64))),
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
        dict(position=p, velocity=v, weight=np.ones((3, 8), F32)),                          # weights are integers
    ]
    for kw in bad:
        with pytest.raises(ValueError, match="RestrictedEnsemble"):
            nb.RestrictedEnsemble(**kw)
    # B * m > 2^26 without 512 MB of zeros: zero-stride views have the shape and cost nothing
    big = np.broadcast_to(np.zeros((1, 1, 2), F32), (3, (1 << 26) // 3 + 1, 2))
    with pytest.raises(ValueError, match=r"RestrictedEnsemble.*tracers.*2\^26"):
        nb.RestrictedEnsemble(p, v, tracers=(big, big))
    bodies = np.broadcast_to(np.zeros((1, 1, 2), F32), ((1 << 14) + 1, 4096, 2))
    with pytest.raises(ValueError, match=r"RestrictedEnsemble.*2\^26"):
        nb.RestrictedEnsemble(bodies, bodies)
    with pytest.raises(ValueError):
        nb.RestrictedEnsemble(p, v, tracers=tr, arith="double")
    assert not made


def test_checked_tracers_accepts_what_the_handle_takes(nb):
    from nbody_simulation_amd.ensemble import _checked_tracers
    assert _checked_tracers(None, 4) == (0, None, None)
    m, tp, tv = _checked_tracers((np.ones((2, 7, 2), F32)[:, ::2], np.ones((2, 4, 2), F32)), 2)
    assert m == 4 and tp.flags.c_contiguous and tp.shape == tv.shape == (2, 4, 2)
    m, tp, tv = _checked_tracers((_z(5, 2), _z(5, 2)), 1)                # one world: [m, 2]
    assert m == 5 and tp.shape == tv.shape == (1, 5, 2)
    m, tp, tv = _checked_tracers((_z(2, 0, 2), _z(2, 0, 2)), 2)          # m = 0 removes them
    assert m == 0
