"""The watched sweep (nbody_wsweep_*, the classes' watch_sweep()) without a GPU: the nine declared names in both libraries and
in the binding under a prefix of their own, NULL-handle calls, the Python argument checks — which raise before any library call
— nbody_wsweep_plan against the three-line sample rule of tests/_wsweep_scene.py, and the proof that the scene and the parameters
of tests/test_gpu_ensemble_wsweep.py can tell the contract from its neighbours.  For that proof every world of the smallest
multi-body shape (six worlds of two bodies) is stepped by the oracle under its own delta and clamp, and the restatement
(tests/_watch_restatement.py) folds its trajectory: under the world's own schedule, and under each rival — a neighbour's stride,
params.clamp as the default limit, sampling on after steps[k], a launch-wide `first` — which must change some world's rows."""
import ctypes
import itertools
import re

import numpy as np
import pytest

import _watch_restatement as W
import _wsweep_scene as Q
from _wsweep_scene import CLAMP, DELTA, HEIGHT, N_STEPS, PARAM_CLAMP, STEPS, STRIDE, WORLDS

NTH = 16
HANDLES = ("ensemble", "ensemble64", "ragged", "ragged64", "restricted", "restricted64", "rr", "rr64")
NAMES = ["nbody_wsweep_" + h for h in HANDLES] + ["nbody_wsweep_plan"]
CLASSES = [("Ensemble", False), ("Ensemble64", False), ("RaggedEnsemble", False), ("RaggedEnsemble64", False), ("RestrictedEnsemble", True),
           ("RestrictedEnsemble64", True), ("RaggedRestrictedEnsemble", True), ("RaggedRestrictedEnsemble64", True)]
I32 = ctypes.POINTER(ctypes.c_int32)


def test_the_header_declares_both_libraries_export_and_the_binding_binds_the_nine_names(nb):
    C = nb._capi
    declared = C.declared_symbols()
    assert sorted(s for s in declared if s.startswith("nbody_wsweep_")) == sorted(NAMES)        # these and no other
    assert sorted(s for s in C._SIGS if s.startswith("nbody_wsweep_")) == sorted(NAMES)
    assert sorted(C._SIGS) == declared
    for path in (C.LIB_PATH, C.LAB_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in NAMES if not hasattr(lib, s)], path
    # the prefix is its own: none of the nine falls into the watch's, the sweep's or a handle's closed set of names
    assert not [s for s in NAMES if s.startswith(("nbody_watch_", "nbody_sweep_") + tuple(f"nbody_{h}_" for h in HANDLES))]
    with open(C.HEADER_PATH) as f:
        head = f.read()
    assert int(re.search(r"#define\s+NBODY_ABI_VERSION\s+(\d+)", head).group(1)) == 3 == C.ABI_VERSION    # new symbols only
    with open(C.HEADER_PATH.replace("nbody_hip.h", "nbody_ensemble.h")) as f:
        ens = f.read()
    for h in HANDLES:
        real, rows = ("double", "f64") if h.endswith("64") else ("float", "f32")
        assert re.search(rf"int\s+nbody_wsweep_{h}\s*\(\s*nbody_{h}\s*\*\s*e,\s*uint32_t\s+flags,\s*const\s+{real}\s*\*\s*delta,\s*const\s+float\s*\*"
                         rf"\s*clamp,\s*const\s+int32_t\s*\*\s*steps,\s*int\s+n_steps,\s*const\s+int32_t\s*\*\s*stride[^,]*,\s*const\s+float\s*\*"
                         rf"\s*limit2[^,]*,\s*uint32_t\s+height,\s*nbody_world_watch\s*\*\s*out[^,]*,\s*const\s+nbody_watch_rows_{rows}\s*\*\s*rows"
                         r"[^,]*,\s*nbody_counting\s*\*\s*counter\s*\)\s*;", ens), h
        res, args = C._SIGS["nbody_wsweep_" + h]
        assert res is ctypes.c_int and len(args) == 12
        assert args[2] is ctypes.POINTER(ctypes.c_double if h.endswith("64") else ctypes.c_float), h
    assert "a watched sweep with a delta" not in ens                          # the watch's "Not offered" no longer lists it
    for cls, _ in CLASSES:
        assert callable(getattr(nb, cls).watch_sweep), cls
    assert callable(nb.watch_sweep_plan)


@pytest.mark.parametrize("which", ["product", "lab"])
def test_a_null_handle_is_invalid_without_a_device(nb, which):
    C = nb._capi
    lib = C._load(which)
    out = np.zeros(3, nb.WATCH_DTYPE)
    steps, stride = np.full(3, 1, np.int32), np.full(3, 1, np.int32)
    for h in HANDLES:
        call = getattr(lib, "nbody_wsweep_" + h)
        delta = np.full(3, 0.1, np.float64 if h.endswith("64") else np.float32)
        ptr = delta.ctypes.data_as(C._SIGS["nbody_wsweep_" + h][1][2])
        assert call(None, 0, ptr, None, steps.ctypes.data_as(I32), 1, stride.ctypes.data_as(I32), None, 0, C._ptr(out), None, None) == C.ERR_INVALID
        assert call(None, 3, None, None, None, 0, None, None, 0, None, None, None) == C.ERR_INVALID
    assert not out.view(np.uint8).any()


class _NoLibrary:
    """Stands where a class keeps its handle: any use of it is a library call."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was touched: {name}")


@pytest.mark.parametrize("cls_name,with_tracers", CLASSES)
def test_the_python_arguments_are_checked_before_the_library_is_reached(nb, cls_name, with_tracers):
    cls = getattr(nb, cls_name)
    e = object.__new__(cls)
    e.h, e._n_worlds = _NoLibrary(), 4
    try:
        good = [0.1, 0.2, 0.3, 0.4]
        bad = [("delta", dict(delta=None)), ("delta", dict(delta=[0.1, 0.2, 0.3])), ("delta", dict(delta=0.1)),
               ("clamp", dict(clamp=[1e-3] * 5)),
               ("steps", dict(steps=[1, 2, 3])), ("steps", dict(steps=[1, 2, 3, 4], n_steps=3)),       # a steps[k] > n_steps
               ("steps", dict(steps=[1, 2, -1, 3])), ("n_steps", dict(n_steps=-1)), ("n_steps", dict(n_steps=1.5)),
               ("stride", dict(stride=[1, 2, 3])), ("stride", dict(stride=[1, 2, 3, 4, 5])),            # a wrong length
               ("stride", dict(stride=0)), ("stride", dict(stride=[1, 2, 0, 1])), ("stride", dict(stride=[1, -2, 3, 1])),   # < 1
               ("stride", dict(stride=2.0)), ("stride", dict(stride=[1, 2, 3, 1 << 31])), ("stride", dict(stride=[[1, 2], [3, 4]])),
               ("limit2", dict(limit2=[1.0, 2.0])), ("limit2", dict(limit2=1.0)),
               ("height", dict(height=-1)), ("height", dict(height=(1 << 24) + 1)),
               ("rows", dict(rows=1)), ("resume", dict(resume="yes"))]
        if with_tracers:
            bad += [("tracers", dict(tracers=1))]
        for arg, kw in bad:
            args = dict(delta=good)
            args.update(kw)
            with pytest.raises(ValueError, match=rf"{cls_name}\.watch_sweep: {arg}\b"):
                e.watch_sweep(**args)
        with pytest.raises(ValueError, match=r"steps\[3\].*world 3"):
            e.watch_sweep(good, steps=[1, 2, 3, 4], n_steps=3)
        with pytest.raises(ValueError, match=r"stride\[2\].*world 2"):
            e.watch_sweep(good, stride=[1, 2, 0, 1])
        if not with_tracers:
            with pytest.raises(TypeError):
                e.watch_sweep(good, tracers=True)
        # and a valid call reaches the handle with the arrays cast and the defaults filled in
        seen = {}

        class Handle:
            def watch_sweep(self, *a):
                seen["args"] = a
                return np.zeros(4, nb.WATCH_DTYPE), None

        e.h = Handle()
        e.watch_sweep(np.array(good, np.float64), clamp=[1e-3, 1e-2, 4e-6, 0.0], steps=[0, 1, 2, 3], stride=2, rows=False)
        delta, clamp, steps, n_steps, stride, limit2, height, tracers, resume, rows, counter = seen["args"]
        assert delta.dtype == e._dtype and clamp.dtype == np.float32 and steps.dtype == np.int32 and n_steps == 3     # max(steps)
        assert stride.dtype == np.int32 and list(stride) == [2] * 4 and limit2 is None and height == 0
        assert (tracers, resume, rows, counter) == (False, False, False, None)
        e.watch_sweep(good, stride=np.array([1, 2, 3, (1 << 31) - 1]), rows=False)
        assert seen["args"][2] is None and seen["args"][3] == 1 and list(seen["args"][4]) == [1, 2, 3, (1 << 31) - 1]
    finally:
        e.h = None    # (nothing for __del__ to close)


# ---- nbody_wsweep_plan against the sample rule
def _plan_raw(C, n_worlds, steps, n_steps, stride, flags, want_samples=True, want_launches=True):
    samples = np.full(max(n_worlds, 1), -7, np.int64)
    launches = ctypes.c_int64(-7)
    rc = C.load().nbody_wsweep_plan(n_worlds, None if steps is None else steps.ctypes.data_as(I32), n_steps,
                                    None if stride is None else stride.ctypes.data_as(I32), flags,
                                    C._ptr(samples) if want_samples else None, ctypes.byref(launches) if want_launches else None)
    return rc, samples, launches.value


def _plan_restated(n_worlds, steps, n_steps, stride, resume):
    steps = [n_steps] * n_worlds if steps is None else [int(v) for v in steps]
    stride = [1] * n_worlds if stride is None else [int(v) for v in stride]
    samples = [sum(Q.takes(s, steps[k], stride[k], resume) for s in range(n_steps + 1)) for k in range(n_worlds)]
    launches = sum(any(Q.takes(s, steps[k], stride[k], resume) for k in range(n_worlds)) for s in range(n_steps + 1))
    return samples, launches


@pytest.mark.parametrize("resume", [False, True])
def test_the_plan_is_the_sample_rule(nb, resume):
    C = nb._capi
    flags = C.WATCH_RESUME if resume else 0
    top = (1 << 31) - 1
    for n_steps in (0, 1, 5, 12):
        # every combination of steps in {0, 1, n_steps} and stride in {1, 2, stride > steps, 2^31 - 1}, one world each, in one call
        combos = [(st, sd) for st in sorted({0, min(1, n_steps), n_steps}) for sd in (1, 2, st + 1, top)]
        steps, stride = (np.array(v, np.int32) for v in zip(*combos))
        rc, samples, launches = _plan_raw(C, len(combos), steps, n_steps, stride, flags)
        want = _plan_restated(len(combos), steps, n_steps, stride, resume)
        assert rc == 0 and (list(samples), launches) == want, (n_steps, list(samples), launches, want)
        assert list(samples) == [st // sd + (0 if resume else 1) for st, sd in combos]                    # the header's formula
        for k, (st, sd) in enumerate(combos):                                                             # and each world alone
            rc, one, launches = _plan_raw(C, 1, steps[k:k + 1], n_steps, stride[k:k + 1], flags)
            assert rc == 0 and (list(one), launches) == _plan_restated(1, [st], n_steps, [sd], resume), (n_steps, st, sd)
        # NULL arrays: steps = n_steps and stride = 1 in every world; either output may be NULL
        for s_arr, d_arr in itertools.product((None, steps), (None, stride)):
            rc, samples, launches = _plan_raw(C, len(combos), s_arr, n_steps, d_arr, flags)
            assert rc == 0 and (list(samples), launches) == _plan_restated(len(combos), s_arr, n_steps, d_arr, resume)
        rc, samples, launches = _plan_raw(C, len(combos), steps, n_steps, stride, flags, want_samples=False)
        assert rc == 0 and (samples == -7).all() and launches == want[1]
        rc, samples, launches = _plan_raw(C, len(combos), steps, n_steps, stride, flags, want_launches=False)
        assert rc == 0 and list(samples) == want[0] and launches == -7
    # a schedule whose union skips some s: {0, 2, 4} and {0, 3, 6} of 0 .. 7 leave 1, 5 and 7 without a launch
    steps, stride = np.array([4, 6], np.int32), np.array([2, 3], np.int32)
    rc, samples, launches = _plan_raw(C, 2, steps, 7, stride, flags)
    assert rc == 0 and (list(samples), launches) == (([2, 2], 4) if resume else ([3, 3], 5))
    assert (list(samples), launches) == _plan_restated(2, steps, 7, stride, resume)
    # the test scene's: under RESUME only the samples 1 .. 5 of the worlds 0, 2 and 3
    rc, samples, launches = _plan_raw(C, WORLDS, STEPS, N_STEPS, STRIDE, flags)
    assert rc == 0 and (list(samples), launches) == (([5, 0, 1, 2, 0, 0], 5) if resume else ([6, 1, 2, 3, 1, 1], 6))
    got = nb.watch_sweep_plan(STEPS, N_STEPS, STRIDE, resume)
    assert list(got[0]) == list(samples) and got[0].dtype == np.int64 and got[1] == launches
    assert nb.watch_sweep_plan([3, 4], 4, 2, resume)[1] == (2 if resume else 3)                          # a scalar stride


def test_the_plan_refuses_what_the_call_refuses_and_writes_nothing(nb):
    C = nb._capi
    ok = np.array([1, 2], np.int32)
    for n_worlds, steps, n_steps, stride, flags in ((0, ok, 2, ok, 0), (-1, ok, 2, ok, 0), (2, ok, -1, ok, 0), (2, ok, 1, ok, 0),
                                                    (2, np.array([1, -1], np.int32), 2, ok, 0), (2, ok, 2, np.array([1, 0], np.int32), 0),
                                                    (2, ok, 2, np.array([-5, 1], np.int32), 0), (2, None, 2, np.array([1, 0], np.int32), 2),
                                                    (2, ok, 2, ok, 4), (2, ok, 2, ok, 0x80000000)):
        rc, samples, launches = _plan_raw(C, n_worlds, steps, n_steps, stride, flags)
        assert rc == C.ERR_INVALID and (samples == -7).all() and launches == -7, (n_worlds, n_steps, flags)
    for bad in (dict(steps=[1, 2], n_steps=1), dict(steps=[1, 2], n_steps=2, stride=[1, 0]), dict(steps=[1, 2], n_steps=2, stride=[1, 2, 3]),
                dict(steps=[[1, 2]], n_steps=2), dict(steps=[1, 2], n_steps=2, resume=1)):
        with pytest.raises(ValueError):
            nb.watch_sweep_plan(**bad)
    rc, samples, launches = _plan_raw(C, 2, ok, 2, ok, C.WATCH_TRACERS | C.WATCH_RESUME)                 # both flags are the call's
    assert rc == 0 and list(samples) == [1, 1] and launches == 2


# ---- the scene of the device test is telling: six worlds of two bodies under the oracle
def _trajectory(orc, w, k, dtype, n_steps, delta=None, clamp=None):
    """World k's positions after 0 .. n_steps oracle steps under its own delta and clamp (or the ones given); every weight is 1."""
    p, v = w["pos"].copy(), w["vel"].copy()
    m = np.ones(p.shape[0], np.uint32)
    out = [p.copy()]
    for _ in range(n_steps):
        p, v = orc.update_direct(p, v, m, delta=float(dtype(DELTA[k] if delta is None else delta)),
                                 clamp=float(CLAMP[k] if clamp is None else clamp), nsteps=1, nthreads=NTH)[:2]
        out.append(p.copy())
    return out


def _fold(traj, samples, limit, dtype):
    """The restated rows of a world that stands still after its trajectory's last state, sampled at `samples`."""
    n = traj[0].shape[0]
    frames = [(s, traj[min(s, len(traj) - 1)], None) for s in samples]
    return W.world(frames, limit, HEIGHT, n, n, dtype)


def _rows_differ(a, b):
    return any(not W.same(a[1][name], b[1][name]) for name in W.ROWS)


@pytest.mark.parametrize("kind", ["ensemble", "ensemble64"])
def test_the_scene_tells_the_contract_from_its_neighbours(orc, kind):
    dtype = Q.KINDS[kind][1]
    worlds, _ = Q.scene(kind, (2,) * WORLDS, (0,) * WORLDS)
    traj = [_trajectory(orc, worlds[k], k, dtype, int(STEPS[k])) for k in range(WORLDS)]
    assert len(set(DELTA)) == WORLDS and all(CLAMP[k] != CLAMP[(k + 1) % WORLDS] for k in range(WORLDS)) and PARAM_CLAMP not in CLAMP

    # the planted pair: the lattice worlds' two bodies stay at a d2 between the smallest and the largest clamp at every sample,
    # so that a limit of clamp[k] and one of another world's clamp, or of params.clamp, answer differently
    lattice = [k for k in range(WORLDS) if k % 3 == 1]
    for k in lattice:
        for p in _trajectory(orc, worlds[k], k, dtype, N_STEPS):
            d = p[1].astype(np.float64) - p[0].astype(np.float64)
            assert float(CLAMP.min()) < float(d @ d) < float(CLAMP.max()), (k, float(d @ d))
    assert {float(CLAMP[k]) for k in lattice} == {float(CLAMP.min()), float(CLAMP.max())}

    for resume in (False, True):
        mine = [_fold(traj[k], Q.taken(int(STEPS[k]), int(STRIDE[k]), resume), CLAMP[k], dtype) for k in range(WORLDS)]
        assert [int(m[0]["samples"]) for m in mine] == ([5, 0, 1, 2, 0, 0] if resume else [6, 1, 2, 3, 1, 1])
        # a neighbour's stride (either neighbour's)
        other = [_fold(traj[k], Q.taken(int(STEPS[k]), int(STRIDE[(k + d) % WORLDS]), resume), CLAMP[k], dtype)
                 for d in (1, WORLDS - 1) for k in range(WORLDS)]
        assert any(_rows_differ(o, mine[i % WORLDS]) for i, o in enumerate(other)), resume
        # params.clamp, not clamp[k], as the limit that limit2=None stands for (under RESUME neither lattice world takes a sample —
        # their schedules are the two that RESUME empties — so it is the call without RESUME that tells the two apart)
        other = [_fold(traj[k], Q.taken(int(STEPS[k]), int(STRIDE[k]), resume), PARAM_CLAMP, dtype) for k in range(WORLDS)]
        assert resume or any(_rows_differ(o, m) for o, m in zip(other, mine))
        # sampling on after steps[k]
        other = [_fold(traj[k], Q.taken(N_STEPS, int(STRIDE[k]), resume), CLAMP[k], dtype) for k in range(WORLDS)]
        assert any(_rows_differ(o, m) for o, m in zip(other, mine)), resume
    # a launch-wide `first`: every world's rows are rewritten at the first s any world samples.  Without RESUME that is s = 0,
    # every world's own first sample; under RESUME it is s = 1, which the worlds 1, 2, 4 and 5 do not take
    first_any = min(min(Q.taken(int(STEPS[k]), int(STRIDE[k]), True), default=N_STEPS + 1) for k in range(WORLDS))
    assert first_any == 1
    mine = [_fold(traj[k], Q.taken(int(STEPS[k]), int(STRIDE[k]), True), CLAMP[k], dtype) for k in range(WORLDS)]
    other = [_fold(traj[k], sorted({first_any} | set(Q.taken(int(STEPS[k]), int(STRIDE[k]), True))), CLAMP[k], dtype) for k in range(WORLDS)]
    assert sum(_rows_differ(o, m) for o, m in zip(other, mine)) >= 2

    # and, as the sweep's own tests show of their scene: one oracle step of world k under its neighbour's delta moves it
    # elsewhere, and under its neighbour's clamp wherever the planted pair is (so the run that is watched is the world's own)
    for k in range(WORLDS):
        nk = (k + 1) % WORLDS
        own = _trajectory(orc, worlds[k], k, dtype, 1)[1]
        assert not W.same(own, _trajectory(orc, worlds[k], k, dtype, 1, delta=DELTA[nk])[1]), k
        if k in lattice:
            assert not W.same(own, _trajectory(orc, worlds[k], k, dtype, 1, clamp=CLAMP[nk])[1]), k
