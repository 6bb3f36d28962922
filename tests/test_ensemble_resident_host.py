"""Resident runs of an ensemble (nbody_resident_*, run() of the four classes without tracers) without a GPU: the five declared
names in both libraries and in the binding and no other name under the prefix, their argument types, NULL-handle calls, the
argument checks of the Python method — which raise before any library call — and nbody_resident_plan, which is host code."""
import ctypes
import os
import re

import numpy as np
import pytest

HANDLES = ("ensemble", "ensemble64", "ragged", "ragged64")
NAMES = ["nbody_resident_" + s for s in HANDLES]
PLAN = "nbody_resident_plan"
CLOSED = ("nbody_ensemble_", "nbody_ensemble64_", "nbody_ragged_", "nbody_ragged64_", "nbody_restricted_", "nbody_restricted64_",
          "nbody_rr_", "nbody_rr64_", "nbody_frames_", "nbody_deltas_", "nbody_delta_", "nbody_sweep_", "nbody_summary_",
          "nbody_encounters_", "nbody_watch_", "nbody_wsweep_")
WITH_RUN = ["Ensemble", "Ensemble64", "RaggedEnsemble", "RaggedEnsemble64"]
WITHOUT_RUN = ["RestrictedEnsemble", "RestrictedEnsemble64", "RaggedRestrictedEnsemble", "RaggedRestrictedEnsemble64"]


def _ensemble_header(C):
    with open(os.path.join(os.path.dirname(C.HEADER_PATH), "nbody_ensemble.h")) as f:
        return f.read()


def test_header_declares_the_five_resident_calls_and_both_libraries_export_them(nb):
    C = nb._capi
    declared = C.declared_symbols()
    assert sorted(s for s in declared if s.startswith("nbody_resident_")) == sorted(NAMES + [PLAN])     # these and no other
    assert sorted(s for s in C._SIGS if s.startswith("nbody_resident_")) == sorted(NAMES + [PLAN])
    assert sorted(C._SIGS) == declared
    for path in (C.LIB_PATH, C.LAB_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in NAMES + [PLAN] if not hasattr(lib, s)], path
    with open(C.HEADER_PATH) as f:
        head = f.read()
    assert int(re.search(r"#define\s+NBODY_ABI_VERSION\s+(\d+)", head).group(1)) == 3 == C.ABI_VERSION    # new symbols only
    assert "nbody_resident" not in head                                     # declared in nbody_ensemble.h, which it includes
    assert not [s for s in NAMES + [PLAN] if s.startswith(CLOSED)]          # a prefix of its own (and not nbody_restricted_)
    ens = _ensemble_header(C)
    assert int(re.search(r"#define\s+NBODY_RESIDENT_MAX_BODIES\s+(\d+)", ens).group(1)) == 256 == C.RESIDENT_MAX_BODIES
    assert int(re.search(r"#define\s+NBODY_RESIDENT_STEPS_PER_LAUNCH\s+(\d+)", ens).group(1)) == 1024 == C.RESIDENT_STEPS_PER_LAUNCH
    assert ens.rstrip().endswith("#endif /* NBODY_ENSEMBLE_H */") and ens.rindex("nbody_wsweep_plan") < ens.index("nbody_resident_")
    section = ens[ens.index("---- resident runs"):]
    assert "Not offered" in section and "tracers" in section and "nbody_ctx" in section and "watch" in section


def test_run_is_on_the_four_classes_without_tracers_only(nb):
    for name in WITH_RUN:
        assert callable(getattr(nb, name).run), name
    for name in WITHOUT_RUN:
        assert not hasattr(getattr(nb, name), "run"), name
    assert "resident_plan" in nb.__all__ and nb.resident_plan is nb.ensemble.resident_plan


@pytest.mark.parametrize("name", ["RestrictedHandle", "Restricted64Handle", "RRHandle", "RR64Handle"])
def test_a_handle_with_tracers_refuses_in_words_before_any_library_call(nb, name):
    C = nb._capi
    h = object.__new__(getattr(C, name))
    h.h = None                                                          # (nothing for __del__ to close)
    h.lib = _NoLibrary()
    with pytest.raises(C.NBodyError, match="resident runs are not offered") as err:
        h.resident(np.zeros(1, h._dtype), None, None, 1)
    assert err.value.code == C.ERR_INVALID


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


@pytest.mark.parametrize("cls", WITH_RUN)
def test_python_checks_raise_before_any_library_call(nb, cls):
    e = object.__new__(getattr(nb, cls))
    e.h = _NoLibrary()
    e._n_worlds = 4
    try:
        good = [0.1, 0.2, 0.3, 0.4]
        bad_calls = [
            ("delta", dict(delta=None)),
            ("delta", dict(delta=[0.1, 0.2, 0.3])),                       # one short
            ("delta", dict(delta=[[0.1, 0.2], [0.3, 0.4]])),
            ("delta", dict(delta=["a", "b", "c", "d"])),
            ("clamp", dict(delta=good, clamp=[1e-3] * 5)),
            ("clamp", dict(delta=0.1, clamp=1e-3)),
            ("steps", dict(delta=good, steps=[1, 2, 3])),
            ("steps", dict(delta=good, steps=[1, 2, 3, 2.5])),            # not integral
            ("steps", dict(delta=good, steps=[1, 2, -1, 3])),             # below 0
            ("steps", dict(delta=good, steps=[1, 2, 3, 4], n_steps=3)),   # above n_steps
            ("n_steps", dict(delta=good, n_steps=-1)),
            ("n_steps", dict(delta=0.1, n_steps=1.5)),
        ]
        for arg, kw in bad_calls:
            with pytest.raises(ValueError, match=rf"{cls}\.run: {arg}\b"):
                e.run(**kw)
        with pytest.raises(ValueError, match=r"steps\[3\].*world 3"):
            e.run(good, steps=[1, 2, 3, 4], n_steps=3)
        # and a valid call reaches the handle, with the arrays cast: delta to the class's dtype, clamp float32, steps int32
        seen = {}

        class Handle:
            def resident(self, delta, clamp, steps, n_steps, counter):
                seen.update(delta=delta, clamp=clamp, steps=steps, n_steps=n_steps, counter=counter)

        e.h = Handle()
        e.run(np.array(good, np.float64), clamp=[1e-3, 1e-2, 4e-6, 0.0], steps=np.array([0.0, 1.0, 2.0, 3.0]))
        assert seen["delta"].dtype == e._dtype and seen["delta"].flags.c_contiguous and seen["delta"].shape == (4,)
        assert seen["clamp"].dtype == np.float32 and seen["steps"].dtype == np.int32
        assert list(seen["steps"]) == [0, 1, 2, 3] and seen["n_steps"] == 3 and seen["counter"] is None   # n_steps = max(steps)
        e.run(0.25, 7)                                                    # a scalar delta is every world's
        assert list(seen["delta"]) == [0.25] * 4 and seen["delta"].dtype == e._dtype and seen["n_steps"] == 7
        assert seen["clamp"] is None and seen["steps"] is None
        e.run(good)
        assert seen["n_steps"] == 1                                       # 1 without steps
    finally:
        e.h = None    # (nothing for __del__ to close)


def _lds(n, f64):
    """The stepping kernels' layout plus the velocities: couples of 24 bytes + 8 n; rows padded to 8 at 20 bytes + 16 n."""
    return (n + 7) // 8 * 8 * 20 + 16 * n if f64 else (n + 1) // 2 * 24 + 8 * n


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_resident_plan(nb, dtype):
    f64 = dtype is np.float64
    assert (_lds(256, False), _lds(256, True), _lds(3, False), _lds(3, True), _lds(1, False), _lds(1, True)) == (5120, 9216, 72, 208, 32, 176)
    assert nb.resident_plan([1, 3, 256], [0, 1024, 1025], 1025, dtype) == dict(n_launches=2, lds_bytes=_lds(256, f64))
    assert nb.resident_plan([1, 3, 256], [0, 1024, 1024], 1025, dtype)["n_launches"] == 1
    assert nb.resident_plan([1, 3, 256], None, 1025, dtype)["n_launches"] == 2          # no steps: every world takes n_steps
    assert nb.resident_plan([1, 3, 256], None, 2049, dtype)["n_launches"] == 3
    for sizes, n_steps in (([1, 3, 256], 1025), ([7], 0), ([200, 5], 1 << 20)):
        assert nb.resident_plan(sizes, [0] * len(sizes), n_steps, dtype) == dict(n_launches=0, lds_bytes=_lds(max(sizes), f64))
    assert nb.resident_plan([3, 2, 1], None, 0, dtype) == dict(n_launches=0, lds_bytes=_lds(3, f64))
    for n in (1, 2, 3, 8, 9, 255, 256):
        assert nb.resident_plan([n], None, 1, dtype) == dict(n_launches=1, lds_bytes=_lds(n, f64))
    for sizes, steps, n_steps in (([1, 257, 3], None, 1), ([3, 0], None, 1), ([], None, 1), ([3, 3], [1, 3], 2), ([3, 3], [-1, 1], 2),
                                  ([3, 3], None, -1)):
        with pytest.raises(ValueError, match="resident_plan"):
            nb.resident_plan(sizes, steps, n_steps, dtype)


@pytest.mark.parametrize("which", ["product", "lab"])
def test_a_refused_plan_writes_nothing(nb, which):
    C = nb._capi
    lib = C._load(which)
    i64, i32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)

    def plan(sizes, steps, n_steps, f64, n_worlds=None):
        sizes = np.array(sizes, np.int64)
        launches, lds = ctypes.c_int32(-7), ctypes.c_int32(-7)
        steps = None if steps is None else np.array(steps, np.int32)
        rc = lib.nbody_resident_plan(len(sizes) if n_worlds is None else n_worlds, sizes.ctypes.data_as(i64),
                                     None if steps is None else steps.ctypes.data_as(i32), n_steps, f64, ctypes.byref(launches), ctypes.byref(lds))
        return rc, launches.value, lds.value

    for f64 in (0, 1):
        assert plan([1, 3, 256], [0, 1024, 1025], 1025, f64) == (C.OK, 2, _lds(256, f64))
        assert plan([1, 257, 256], None, 4, f64) == (C.ERR_INVALID, -7, -7)
        assert plan([1, 3], None, 4, f64, n_worlds=0) == (C.ERR_INVALID, -7, -7)
        assert plan([1, 3], None, 4, f64, n_worlds=-1) == (C.ERR_INVALID, -7, -7)
        assert plan([1, 3], [1, 5], 4, f64) == (C.ERR_INVALID, -7, -7)
        assert plan([1, 3], [-1, 4], 4, f64) == (C.ERR_INVALID, -7, -7)
        assert plan([1, 3], None, -1, f64) == (C.ERR_INVALID, -7, -7)
    assert lib.nbody_resident_plan(2, np.array([3, 4], np.int64).ctypes.data_as(i64), None, 5, 0, None, None) == C.OK   # both outputs may be NULL
    assert lib.nbody_resident_plan(2, None, None, 5, 0, None, None) == C.ERR_INVALID
