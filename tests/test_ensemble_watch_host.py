"""The watch's contract on the CPU (no device): the NumPy restatement (tests/_watch_restatement.py) against hand-computed
straight-line cases, nb.watch_merge against the restatement's own merge, the record's layout, the header and the bindings, the
NULL-handle refusals and the Python argument checks.  And the proof that the scenes of tests/test_gpu_ensemble_watch.py can tell
the contract's tie rules from their alternatives: on the lattice world at rest, a fold in which the latest sample stands gives
other min_sample values, and a walk in which the highest source index stands gives other min_index values."""
import ctypes
import re

import numpy as np
import pytest

import _watch_restatement as W

F32, F64 = np.float32, np.float64
NEVER = W.NEVER
HANDLES = ("ensemble", "ensemble64", "ragged", "ragged64", "restricted", "restricted64", "rr", "rr64")


def run(pos, vel, n_steps, stride=1, resume=False, limit2=1.5, height=64, delta=0.5, tracers=None, **rival):
    """The restated watch of one world on straight lines: pos, vel lists or arrays [n, 2]; tracers None or (tpos, tvel)."""
    pos, vel = np.asarray(pos), np.asarray(vel)
    bodies = W.ballistic(pos, vel, delta, n_steps)
    samples = W.taken(n_steps, stride, resume)
    if tracers is None:
        return W.world(W.frames_of(samples, bodies), limit2, height, pos.shape[0], pos.shape[0], pos.dtype, **rival)
    tpos = W.ballistic(np.asarray(tracers[0]), np.asarray(tracers[1]), delta, n_steps)
    return W.world(W.frames_of(samples, tpos, bodies), limit2, height, tpos[0].shape[0], pos.shape[0], pos.dtype, **rival)


def pair(dtype, x1, y1=1.0):
    """Body 0 at the origin moving one unit per step along x, body 1 at rest at (x1, y1): d2 = (x1 - s)^2 + y1^2 at sample s."""
    return np.array([[0, 0], [x1, y1]], dtype), np.array([[2, 0], [0, 0]], dtype)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_the_restatement_gives_the_hand_computed_numbers(dtype):
    pos, vel, tpos, tvel = W.hand_world(dtype)
    h = W.HAND
    got = run(pos, vel, h["n_steps"], limit2=h["limit2"], height=h["height"], delta=h["delta"])
    want = W.hand_expected("bodies", dtype)
    assert W.same_world(got, want), W.diff(got, want)
    got = run(pos, vel, h["n_steps"], limit2=h["limit2"], height=h["height"], delta=h["delta"], tracers=(tpos, tvel))
    want = W.hand_expected("tracers", dtype)
    assert W.same_world(got, want), W.diff(got, want)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_the_edges_of_the_contract_one_line_each(dtype):
    inf = np.inf
    # an approach whose minimum is at a middle sample: d2 = 10 5 2 1 2 5
    rec, rows = run(*pair(dtype, 3.0), 5)
    assert (rows["min_d2"][0], rows["min_index"][0], rows["min_sample"][0]) == (1.0, 1, 3) and rec["min_sample"] == 3
    # a tie in time: d2 = 7.25 3.25 1.25 1.25 3.25 7.25, the earliest sample stands
    rec, rows = run(*pair(dtype, 2.5), 5)
    assert (rows["min_d2"][0], rows["min_sample"][0], rec["min_sample"], rec["min_row"]) == (1.25, 2, 2, 0)
    # a tie between sources: bodies 1 and 2 at the same distance of body 0 at rest, the lowest index stands
    rec, rows = run(np.array([[0, 0], [-1, 0], [1, 0]], dtype), np.zeros((3, 2), dtype), 2)
    assert list(rows["min_index"]) == [1, 0, 0] and rec["min_source"] == 1
    # a target that never has a live pair: alone, or on top of its only neighbour all the way
    for n in (1, 2):
        rec, rows = run(np.full((n, 2), 5, dtype), np.full((n, 2), 2, dtype), 3)
        assert list(rows["min_index"]) == [-1] * n and list(rows["min_sample"]) == [NEVER] * n and np.isposinf(rows["min_d2"]).all()
        assert (rec["isolated_rows"], rec["min_row"], rec["min_source"], rec["min_sample"], rec["min_d2"]) == (n, -1, -1, -1, inf)
    # d2 overflowing to +inf as the first live pair: it stands with its index and its sample, and a finite one replaces it
    big = dtype(2.0 ** 126) if dtype == F32 else dtype(2.0 ** 1022)
    far = np.array([[-big, 0], [big, 0]], dtype)
    rec, rows = run(far, np.zeros((2, 2), dtype), 2, limit2=inf)
    assert list(rows["min_index"]) == [1, 0] and list(rows["min_sample"]) == [0, 0] and np.isposinf(rows["min_d2"]).all()
    assert rec["isolated_rows"] == 0 and rec["min_row"] == 0 and rec["close_rows"] == 0          # +inf is not below +inf
    frames = [(0, far, None), (1, np.array([[0, 0], [2, 0]], dtype), None)]
    rec, rows = W.world(frames, 1.5, 64, 2, 2, dtype)
    assert list(rows["min_d2"]) == [4, 4] and list(rows["min_sample"]) == [1, 1]
    # a NaN limit and a 0 limit are never close, +inf is close wherever a finite d2 is
    for limit, close in ((np.nan, 0), (0.0, 0), (inf, 6)):
        rec, rows = run(*pair(dtype, 3.0), 5, limit2=limit)
        assert list(rows["close_samples"]) == [close] * 2 and rec["close_row_samples"] == 2 * close
        assert list(rows["first_close"]) == [0 if close else NEVER] * 2 and rec["first_close_sample"] == (0 if close else -1)
    # height == 0: every row is out at the first sample; a NaN position is out under any height
    rec, rows = run(*pair(dtype, 3.0), 5, height=0)
    assert list(rows["first_out"]) == [0, 0] and (rec["out_rows"], rec["first_out_sample"]) == (2, 0)
    rec, rows = run(np.array([[np.nan, 1], [3, 1]], dtype), np.zeros((2, 2), dtype), 1, height=1 << 24)
    assert list(rows["first_out"]) == [0, NEVER] and list(rows["min_index"]) == [-1, -1]
    # a stride that does not divide n_steps: the samples 0 2 4 of d2 = 10 5 2 1 2 5 — the minimum at 3 is not seen, 2 stands over 4
    rec, rows = run(*pair(dtype, 3.0), 5, stride=2)
    assert rec["samples"] == 3 and (rows["min_d2"][0], rows["min_sample"][0]) == (2.0, 2)
    # RESUME: sample 0 is left out — d2 = 1.25 0.25 1.25 at the samples 0 1 2, all close, so the close sample 0 is not counted
    rec, rows = run(*pair(dtype, 1.0, 0.5), 2)
    assert rec["samples"] == 3 and list(rows["close_samples"]) == [3, 3] and list(rows["first_close"]) == [0, 0]
    rec, rows = run(*pair(dtype, 1.0, 0.5), 2, resume=True)
    assert rec["samples"] == 2 and list(rows["close_samples"]) == [2, 2] and list(rows["first_close"]) == [1, 1]
    # no step without RESUME is one sample; with RESUME no sample at all
    rec, rows = run(*pair(dtype, 3.0), 0)
    assert rec["samples"] == 1 and list(rows["min_sample"]) == [0, 0]
    rec, rows = run(*pair(dtype, 3.0), 0, resume=True)
    assert (rec["samples"], rec["isolated_rows"], rec["min_row"]) == (0, 2, -1) and list(rows["min_sample"]) == [NEVER] * 2


def test_taken_samples():
    assert W.taken(5) == [0, 1, 2, 3, 4, 5] and W.taken(5, 2) == [0, 2, 4] and W.taken(5, 2, True) == [2, 4]
    assert W.taken(0) == [0] and W.taken(0, 3, True) == [] and W.taken(3, 5, True) == []


def _as_call(world_result, ragged=False):
    """One world's (record, rows) as a one-world `watch()` result."""
    rec, rows = world_result
    out = np.zeros(1, W.DTYPE)
    out[0] = rec
    return out, {name: [rows[name]] if ragged else rows[name][None] for name in W.ROWS}


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_watch_merge_of_a_run_split_at_every_multiple_of_the_stride_is_the_whole(nb, dtype, stride):
    pos, vel, tpos, tvel = W.hand_world(dtype)
    lat, lat_vel = W.static_lattice(dtype)
    n_steps = 7
    for p, v, tr in ((pos, vel, None), (pos, vel, (tpos, tvel)), (lat[:40], lat_vel[:40], None)):
        bodies = W.ballistic(p, v, 0.5, n_steps)
        targets = bodies if tr is None else W.ballistic(tr[0], tr[1], 0.5, n_steps)
        sources = None if tr is None else bodies
        shape = (targets[0].shape[0], p.shape[0], dtype)
        whole = W.world(W.frames_of(W.taken(n_steps, stride), targets, sources), 1.5, 12, *shape)
        for n1 in range(0, n_steps + 1, stride):
            first = W.world(W.frames_of(W.taken(n1, stride), targets, sources), 1.5, 12, *shape)
            rest = [(s - n1, t, src) for s, t, src in W.frames_of([s for s in W.taken(n_steps, stride) if s > n1], targets, sources)]
            second = W.world(rest, 1.5, 12, *shape)
            assert second[0]["samples"] == len(W.taken(n_steps - n1, stride, True))
            mine = W.merge(first, second, n1)
            assert W.same_world(mine, whole), (n1, W.diff(mine, whole))
            for ragged in (False, True):
                rec, rows = nb.watch_merge(_as_call(first, ragged), _as_call(second, ragged), n1)
                assert rec.dtype == nb.WATCH_DTYPE and rec.shape == (1,)
                got = (rec[0], {name: rows[name][0] for name in W.ROWS})
                assert W.same_world(got, whole), (n1, ragged, W.diff(got, whole))


def test_watch_merge_checks_its_arguments(nb):
    pos, vel, _, _ = W.hand_world(F32)
    a = _as_call(run(pos, vel, 2))
    with pytest.raises(ValueError, match="rows"):
        nb.watch_merge((a[0], None), a, 2)
    with pytest.raises(ValueError, match="steps_before"):
        nb.watch_merge(a, a, -1)
    other = _as_call(run(pos[:3], vel[:3], 2))
    with pytest.raises(ValueError, match="same worlds"):
        nb.watch_merge(a, other, 2)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_the_lattice_at_rest_tells_the_tie_rules_from_their_alternatives(dtype):
    pos, vel = W.static_lattice(dtype)
    mine = run(pos, vel, 5, limit2=1.5, height=8)
    latest = run(pos, vel, 5, limit2=1.5, height=8, latest=True)
    highest = run(pos, vel, 5, limit2=1.5, height=8, highest=True)
    assert (mine[1]["min_sample"] == 0).all() and (latest[1]["min_sample"] == 5).all()            # every target's minimum is tied in time
    assert mine[0]["min_sample"] == 0 and latest[0]["min_sample"] == 5
    moved = int((mine[1]["min_index"] != highest[1]["min_index"]).sum())
    assert moved > pos.shape[0] // 2, moved                                                      # most targets have tied sources
    assert W.same(mine[1]["min_d2"], highest[1]["min_d2"]) and W.same(mine[1]["min_d2"], latest[1]["min_d2"])
    assert mine[0]["min_source"] != highest[0]["min_source"]
    # and the hand-computed world tells the rule in time too: bodies 2 and 3 are tied over the samples 2 and 3
    p, v, _, _ = W.hand_world(dtype)
    assert list(run(p, v, 5)[1]["min_sample"][2:4]) == [2, 2] and list(run(p, v, 5, latest=True)[1]["min_sample"][2:4]) == [3, 3]


def test_the_record_is_thirteen_fields_of_eight_bytes(nb):
    d = nb.WATCH_DTYPE
    assert d.itemsize == 104 and len(d.names) == 13
    assert [d.fields[name][1] for name in d.names] == [8 * i for i in range(13)]
    assert d.names == W.DTYPE.names and d == W.DTYPE
    assert d["min_d2"] == np.float64 and all(d[name] == np.int64 for name in d.names if name != "min_d2")
    assert nb.WATCH_NEVER == 0xffffffff == nb._capi.WATCH_NEVER
    assert ctypes.sizeof(nb._capi.WatchRows) == 6 * ctypes.sizeof(ctypes.c_void_p)


def test_the_header_declares_and_the_binding_binds_the_eight_calls_and_the_structs(nb):
    C = nb._capi
    declared = C.declared_symbols()
    names = ["nbody_watch_" + h for h in HANDLES]
    assert [s for s in declared if s.startswith("nbody_watch_")] == sorted(names)
    assert all(name in C._SIGS for name in names)
    lib = ctypes.CDLL(C.LIB_PATH)
    assert all(hasattr(lib, name) for name in names)
    with open(C.HEADER_PATH.replace("nbody_hip.h", "nbody_ensemble.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for struct in ("nbody_world_watch", "nbody_watch_rows_f32", "nbody_watch_rows_f64"):
        assert re.search(r"typedef struct %s \{[^}]*\} %s;" % (struct, struct), text), struct
    fields = re.search(r"typedef struct nbody_world_watch \{([^}]*)\}", text).group(1)
    assert re.findall(r"(\w+)\s*[,;]", fields) == list(nb.WATCH_DTYPE.names)
    for name, value in (("NBODY_WATCH_TRACERS", "1u"), ("NBODY_WATCH_RESUME", "2u"), ("NBODY_WATCH_NEVER", "0xffffffffu")):
        assert re.search(r"#define %s %s\b" % (name, value), text), name
    assert (C.WATCH_TRACERS, C.WATCH_RESUME) == (1, 2)
    assert re.search(r"#define NBODY_ABI_VERSION 3\b", open(C.HEADER_PATH).read()) and C.ABI_VERSION == 3


@pytest.mark.parametrize("handle", HANDLES)
def test_a_null_handle_is_invalid_without_a_device(nb, handle):
    C = nb._capi
    out = np.zeros(2, nb.WATCH_DTYPE)
    call = getattr(C.load(), "nbody_watch_" + handle)
    assert call(None, 0, 0.5, 1, 1, None, 0, C._ptr(out), None, None) == C.ERR_INVALID
    assert call(None, 3, 0.5, 0, 1, None, 0, None, None, None) == C.ERR_INVALID
    assert not out.view(np.uint8).any()


class _NoLibrary:
    """A handle that must not be reached: the argument checks come first."""

    def watch(self, *a, **k):
        raise AssertionError("the library was reached")


@pytest.mark.parametrize("cls_name,with_tracers", [("Ensemble", False), ("Ensemble64", False), ("RaggedEnsemble", False),
                                                   ("RaggedEnsemble64", False), ("RestrictedEnsemble", True),
                                                   ("RestrictedEnsemble64", True), ("RaggedRestrictedEnsemble", True),
                                                   ("RaggedRestrictedEnsemble64", True)])
def test_the_python_arguments_are_checked_before_the_library_is_reached(nb, cls_name, with_tracers):
    cls = getattr(nb, cls_name)
    ens = cls.__new__(cls)                       # no device: the checks need the number of worlds and the dtype alone
    ens.h, ens._n_worlds = _NoLibrary(), 3
    bad = [dict(delta="0.1"), dict(delta=None), dict(delta=True), dict(n_steps=-1), dict(n_steps=1.5), dict(n_steps=True), dict(n_steps=1 << 31),
           dict(stride=0), dict(stride=-2), dict(stride=2.0), dict(height=-1), dict(height=(1 << 24) + 1), dict(height=1.0),
           dict(limit2=[1.0, 2.0]), dict(limit2=1.0), dict(limit2=["a", "b", "c"]), dict(limit2=np.zeros((3, 1))),
           dict(rows=1), dict(resume="yes"), dict(rows=None)]
    if with_tracers:
        bad += [dict(tracers=1), dict(tracers=None)]
    for kw in bad:
        args = dict(delta=0.5)
        args.update(kw)
        with pytest.raises(ValueError, match=cls_name + r"\.watch: " + next(iter(kw))):
            ens.watch(**args)
    if not with_tracers:
        with pytest.raises(TypeError):
            ens.watch(0.5, tracers=True)
    ens.h = None
