"""Sweeps of an ensemble (nbody_sweep_*, the classes' sweep()) without a GPU: the eight declared names in both libraries and in
the binding and no other name under the prefix, their argument types, NULL-handle calls, the argument checks of the Python
method — which raise before any library call — and the header's "Not offered" lists."""
import ctypes
import os
import re

import numpy as np
import pytest

HANDLES = ("ensemble", "ensemble64", "ragged", "ragged64", "restricted", "restricted64", "rr", "rr64")
NAMES = ["nbody_sweep_" + s for s in HANDLES]


def _ensemble_header(C):
    with open(os.path.join(os.path.dirname(C.HEADER_PATH), "nbody_ensemble.h")) as f:
        return f.read()


def test_header_declares_the_eight_sweep_calls_and_both_libraries_export_them(nb):
    C = nb._capi
    declared = C.declared_symbols()
    assert sorted(s for s in declared if s.startswith("nbody_sweep_")) == sorted(NAMES)        # these and no other
    assert sorted(s for s in C._SIGS if s.startswith("nbody_sweep_")) == sorted(NAMES)
    assert sorted(C._SIGS) == declared
    for path in (C.LIB_PATH, C.LAB_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in NAMES if not hasattr(lib, s)], path
    with open(C.HEADER_PATH) as f:
        head = f.read()
    assert int(re.search(r"#define\s+NBODY_ABI_VERSION\s+(\d+)", head).group(1)) == 3 == C.ABI_VERSION    # new symbols only
    assert "nbody_sweep" not in head                                        # declared in nbody_ensemble.h, which it includes
    # the prefix is its own: none of the eight falls into a handle's closed set of names, the frames' or the delta streams'
    assert not [s for s in NAMES if s.startswith(("nbody_ensemble_", "nbody_ensemble64_", "nbody_ragged_", "nbody_ragged64_",
                                                  "nbody_restricted_", "nbody_restricted64_", "nbody_rr_", "nbody_rr64_",
                                                  "nbody_frames_", "nbody_deltas_", "nbody_delta_"))]
    for cls in (nb.Ensemble, nb.Ensemble64, nb.RaggedEnsemble, nb.RaggedEnsemble64, nb.RestrictedEnsemble, nb.RestrictedEnsemble64,
                nb.RaggedRestrictedEnsemble, nb.RaggedRestrictedEnsemble64):
        assert callable(cls.sweep), cls


def test_f64_handles_take_double_deltas_and_all_take_float_clamps(nb):
    C = nb._capi
    ens = _ensemble_header(C)
    for h, name in zip(HANDLES, NAMES):
        real, ctype = ("double", ctypes.c_double) if h.endswith("64") else ("float", ctypes.c_float)
        assert re.search(rf"int\s+{name}\s*\(\s*nbody_{h}\s*\*\s*e,\s*const\s+{real}\s*\*\s*delta,\s*const\s+float\s*\*\s*clamp,\s*"
                         r"const\s+int32_t\s*\*\s*steps,\s*int\s+n_steps,\s*nbody_counting\s*\*\s*counter\s*\)\s*;", ens), name
        res, args = C._SIGS[name]
        assert res is ctypes.c_int and len(args) == 6
        assert args[1] is ctypes.POINTER(ctype), name
        assert args[2] is ctypes.POINTER(ctypes.c_float), name
        assert args[3] is ctypes.POINTER(ctypes.c_int32), name
        assert args[4] is ctypes.c_int


@pytest.mark.parametrize("which", ["product", "lab"])
def test_null_handle_calls(nb, which):
    C = nb._capi
    lib = C._load(which)
    clamp = np.full(3, 0.001, np.float32)
    steps = np.full(3, 1, np.int32)
    counter = C.Counting()
    for h, name in zip(HANDLES, NAMES):
        delta = np.full(3, 0.1, np.float64 if h.endswith("64") else np.float32)
        ptr = delta.ctypes.data_as(C._SIGS[name][1][1])
        assert getattr(lib, name)(None, ptr, clamp.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                  steps.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1, ctypes.byref(counter)) == C.ERR_INVALID, name
        assert getattr(lib, name)(None, None, None, None, 0, None) == C.ERR_INVALID, name
        assert getattr(lib, name)(None, ptr, None, None, -1, None) == C.ERR_INVALID, name
    assert counter.sum_gravity == 0.0


class _NoLibrary:
    """Stands where a class keeps its handle: any use of it is a library call."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was touched: {name}")


def _unbuilt(cls, worlds):
    obj = object.__new__(cls)
    obj.h = _NoLibrary()
    obj._n_worlds = worlds
    return obj


CLASSES = ["Ensemble", "Ensemble64", "RaggedEnsemble", "RaggedEnsemble64", "RestrictedEnsemble", "RestrictedEnsemble64",
           "RaggedRestrictedEnsemble", "RaggedRestrictedEnsemble64"]


@pytest.mark.parametrize("cls", CLASSES)
def test_python_checks_raise_before_any_library_call(nb, cls):
    e = _unbuilt(getattr(nb, cls), 4)
    try:
        good = [0.1, 0.2, 0.3, 0.4]
        bad_calls = [
            ("delta", dict(delta=None)),
            ("delta", dict(delta=[0.1, 0.2, 0.3])),                       # one short
            ("delta", dict(delta=0.1)),                                   # a scalar is not one value per world
            ("delta", dict(delta=[[0.1, 0.2], [0.3, 0.4]])),
            ("delta", dict(delta=["a", "b", "c", "d"])),
            ("clamp", dict(delta=good, clamp=[1e-3] * 5)),
            ("clamp", dict(delta=good, clamp=1e-3)),
            ("steps", dict(delta=good, steps=[1, 2, 3])),
            ("steps", dict(delta=good, steps=[1, 2, 3, 2.5])),            # not integral
            ("steps", dict(delta=good, steps=[1, 2, 3, np.nan])),
            ("steps", dict(delta=good, steps=[1, 2, -1, 3])),             # below 0
            ("steps", dict(delta=good, steps=[1, 2, 3, 4], n_steps=3)),   # above n_steps
            ("steps", dict(delta=good, steps=[1, 2, 3, 1 << 31])),
            ("n_steps", dict(delta=good, n_steps=-1)),
            ("n_steps", dict(delta=good, n_steps=1.5)),
        ]
        for arg, kw in bad_calls:
            with pytest.raises(ValueError, match=rf"{cls}\.sweep: {arg}\b"):
                e.sweep(**kw)
        with pytest.raises(ValueError, match=r"steps\[3\].*world 3"):
            e.sweep(good, steps=[1, 2, 3, 4], n_steps=3)
        # and a valid call reaches the handle, with the arrays cast: delta to the class's dtype, clamp float32, steps int32
        seen = {}

        class Handle:
            def sweep(self, delta, clamp, steps, n_steps, counter):
                seen.update(delta=delta, clamp=clamp, steps=steps, n_steps=n_steps, counter=counter)

        e.h = Handle()
        e.sweep(np.array(good, np.float64), clamp=[1e-3, 1e-2, 4e-6, 0.0], steps=np.array([0.0, 1.0, 2.0, 3.0]))
        assert seen["delta"].dtype == e._dtype and seen["delta"].flags.c_contiguous and seen["delta"].shape == (4,)
        assert seen["clamp"].dtype == np.float32 and seen["steps"].dtype == np.int32
        assert list(seen["steps"]) == [0, 1, 2, 3] and seen["n_steps"] == 3 and seen["counter"] is None   # n_steps = max(steps)
        e.sweep(good)
        assert seen["clamp"] is None and seen["steps"] is None and seen["n_steps"] == 1                   # 1 without steps
        e.sweep(good, steps=[0, 1, 1, 0], n_steps=5)
        assert seen["n_steps"] == 5 and list(seen["steps"]) == [0, 1, 1, 0]
    finally:
        e.h = None    # (nothing for __del__ to close)


def test_not_offered_lists_no_longer_name_a_per_world_delta_or_clamp(nb):
    ens = _ensemble_header(nb._capi)
    assert "a per-world delta or clamp" not in ens
    assert not re.search(r"per-world\s+(delta|clamp)", ens)
    lists = re.findall(r"Not offered[^:]*:(.*?)(?:\*/|\n \*   [A-Z])", ens, flags=re.S)
    assert len(lists) >= 8
    for text in lists:
        assert not re.search(r"per-world\s+(delta|clamp|time step)", text), text
    assert "nbody_sweep_" in ens and "stands still" in ens
