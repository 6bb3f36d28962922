"""Encounters of an ensemble (nbody_encounters_*, the classes' encounters(), nb.encounters_of) without a GPU: the ten declared
names in both libraries and in the binding, no other name under the prefix, the ABI version, the record's size and offsets from a
C99 program, NULL-handle calls, the Python checks, nbody_encounters_of_f32 / _of_f64 against the NumPy restatement of the contract
(tests/_encounters_restatement.py) on the scene of tests/_encounters_scene.py, what every plant is there for, and the visibility
conditions: on these very rows another tie rule gives other indices and a fused d2 other bits, so the GPU tests can see both."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _encounters_restatement as R
import _encounters_scene as S

HANDLES = ("ensemble", "ensemble64", "ragged", "ragged64", "restricted", "restricted64", "rr", "rr64")
CALLS = ["nbody_encounters_" + s for s in HANDLES]
NAMES = CALLS + ["nbody_encounters_of_f32", "nbody_encounters_of_f64"]
CLASSES = ["Ensemble", "Ensemble64", "RaggedEnsemble", "RaggedEnsemble64", "RestrictedEnsemble", "RestrictedEnsemble64",
           "RaggedRestrictedEnsemble", "RaggedRestrictedEnsemble64"]
WITH_TRACERS = {"RestrictedEnsemble", "RestrictedEnsemble64", "RaggedRestrictedEnsemble", "RaggedRestrictedEnsemble64"}
FIELDS = ["rows", "sources", "live_pairs", "skipped_pairs", "close_pairs", "close_rows", "isolated_rows", "min_row", "min_source",
          "min_d2", "max_nn_row", "max_nn_d2"]
COUNTS = [0, 1, 2, 64, 65, 255, 256, 257, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 4096]
DTYPES = [np.float32, np.float64]


def test_header_declares_the_encounter_calls_and_both_libraries_export_them(nb):
    C = nb._capi
    assert len(NAMES) == 10
    declared = C.declared_symbols()
    assert sorted(s for s in declared if s.startswith("nbody_encounters_")) == sorted(NAMES)      # these and no other
    assert sorted(s for s in C._SIGS if s.startswith("nbody_encounters_")) == sorted(NAMES)
    assert sorted(C._SIGS) == declared
    for path in (C.LIB_PATH, C.LAB_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in NAMES if not hasattr(lib, s)], path
        exported = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\bnbody_encounters_\w+", exported))) == sorted(NAMES), path
    with open(C.HEADER_PATH) as f:
        head = f.read()
    assert int(re.search(r"#define\s+NBODY_ABI_VERSION\s+(\d+)", head).group(1)) == 3 == C.ABI_VERSION    # new symbols only
    assert "nbody_encounters" not in head                                   # declared in nbody_ensemble.h, which it includes
    with open(os.path.join(os.path.dirname(C.HEADER_PATH), "nbody_ensemble.h")) as f:
        ens = f.read()
    note = r"\s*(/\*.*?\*/)?\s*"
    for name in CALLS:
        handle = "nbody_" + name[len("nbody_encounters_"):]
        real = "double" if name.endswith("64") else "float"
        assert re.search(rf"int\s+{name}\s*\(\s*{handle}\s*\*\s*e,\s*uint32_t\s+flags,\s*const\s+float\s*\*\s*limit2{note},"
                         rf"\s*nbody_world_encounters\s*\*\s*out{note},\s*int32_t\s*\*\s*nn_index{note},\s*{real}\s*\*\s*nn_d2{note},"
                         rf"\s*uint32_t\s*\*\s*close{note}\)\s*;", ens), name
        assert len(C._SIGS[name][1]) == 7
    for name, real in (("nbody_encounters_of_f32", "float"), ("nbody_encounters_of_f64", "double")):
        assert re.search(rf"int\s+{name}\s*\(\s*int64_t\s+n_targets,\s*const\s+{real}\s*\*\s*target_xy,\s*int64_t\s+n_sources,\s*"
                         rf"const\s+{real}\s*\*\s*source_xy,\s*int\s+self,\s*{real}\s+limit2,\s*nbody_world_encounters\s*\*\s*out,\s*"
                         rf"int32_t\s*\*\s*nn_index{note},\s*{real}\s*\*\s*nn_d2{note},\s*uint32_t\s*\*\s*close{note}\)\s*;", ens), name
        assert len(C._SIGS[name][1]) == 10
    assert re.search(r"#define\s+NBODY_ENCOUNTERS_TRACERS\s+1u", ens) and C.ENCOUNTERS_TRACERS == 1
    # the prefix is its own: it is a prefix of no other set of names and none is a prefix of it
    others = ("nbody_ensemble_", "nbody_ensemble64_", "nbody_ragged_", "nbody_ragged64_", "nbody_restricted_", "nbody_restricted64_",
              "nbody_rr_", "nbody_rr64_", "nbody_frames_", "nbody_deltas_", "nbody_delta_", "nbody_sweep_", "nbody_summary_")
    assert not [s for s in NAMES if s.startswith(others)]
    assert not [s for s in declared if s.startswith("nbody_encounters") and s not in NAMES]
    # the section's parts, and what the header says is not offered
    section = ens[ens.index("encounters of an ensemble"):]
    for part in ("Arithmetic.", "Fields.", "Tie rules.", "Calls.", "Tracers.", "Refusals.", "Not offered:", "order-free", "Two launches"):
        assert part in section, part
    for words in ("tracer-tracer pairs", "k nearest", "minimum over the steps", "device-pointer variant", "nbody_ctx contexts"):
        assert words in section[section.index("Not offered:"):], words
    assert "encounters_of" in nb.__all__ and nb.encounters_of is nb.ensemble.encounters_of and nb.ENCOUNTERS_DTYPE is C.ENCOUNTERS_DTYPE
    for cls in CLASSES:
        assert callable(getattr(nb, cls).encounters), cls


def test_the_record_is_96_bytes_with_the_dtypes_offsets_in_c99(nb, tmp_path):
    C = nb._capi
    assert list(nb.ENCOUNTERS_DTYPE.names) == FIELDS == list(R.DTYPE.names)
    assert nb.ENCOUNTERS_DTYPE.itemsize == 96 == R.DTYPE.itemsize
    assert [nb.ENCOUNTERS_DTYPE.fields[f][1] for f in FIELDS] == [8 * i for i in range(12)] == [R.DTYPE.fields[f][1] for f in FIELDS]
    kinds = [np.dtype(np.float64) if f in ("min_d2", "max_nn_d2") else np.dtype(np.int64) for f in FIELDS]
    assert [nb.ENCOUNTERS_DTYPE.fields[f][0] for f in FIELDS] == kinds == [R.DTYPE.fields[f][0] for f in FIELDS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nbody_hip.h"\nint main(void) {\n'
                   '  printf("%u", (unsigned)sizeof(nbody_world_encounters));\n' +
                   "".join(f'  printf(" %u", (unsigned)offsetof(nbody_world_encounters, {f}));\n' for f in FIELDS) +
                   '  printf(" %u\\n", (unsigned)NBODY_ENCOUNTERS_TRACERS);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    inc = os.path.dirname(C.HEADER_PATH)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", inc, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [96] + [8 * i for i in range(12)] + [1]


@pytest.mark.parametrize("which", ["product", "lab"])
def test_null_handle_calls_and_what_encounters_of_refuses(nb, which):
    C = nb._capi
    lib = C._load(which)
    out = np.zeros(4, nb.ENCOUNTERS_DTYPE)
    out["rows"] = 7
    lim = np.ones(4, np.float32)
    idx = np.zeros(16, np.int32)
    for name in CALLS:
        for flags in (0, 1, 2):
            assert getattr(lib, name)(None, flags, lim.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), C._ptr(out), C._ptr(idx), None,
                                      None) == C.ERR_INVALID, name
        assert getattr(lib, name)(None, 0, None, None, None, None, None) == C.ERR_INVALID, name
    for name, dtype in (("nbody_encounters_of_f32", np.float32), ("nbody_encounters_of_f64", np.float64)):
        call = getattr(lib, name)
        p, q = np.ones((3, 2), dtype), np.zeros((5, 2), dtype)
        assert call(-1, C._ptr(p), 3, C._ptr(p), 0, 1.0, C._ptr(out), None, None, None) == C.ERR_INVALID
        assert call(3, C._ptr(p), -1, C._ptr(p), 0, 1.0, C._ptr(out), None, None, None) == C.ERR_INVALID
        assert call(3, C._ptr(p), 5, C._ptr(q), 0, 1.0, None, None, None, None) == C.ERR_INVALID
        assert call(3, None, 5, C._ptr(q), 0, 1.0, C._ptr(out), None, None, None) == C.ERR_INVALID
        assert call(3, C._ptr(p), 5, None, 0, 1.0, C._ptr(out), None, None, None) == C.ERR_INVALID
        assert call(3, C._ptr(p), 5, C._ptr(q), 1, 1.0, C._ptr(out), None, None, None) == C.ERR_INVALID      # self needs equal counts
        assert (out["rows"] == 7).all() and not out["sources"].any()
        one = np.zeros(1, nb.ENCOUNTERS_DTYPE)
        assert call(0, None, 0, None, 1, 1.0, C._ptr(one), None, None, None) == C.OK                         # no rows need no arrays
        assert R.same(one[0], R.segment(np.zeros((0, 2), dtype), None, 1.0)[0])
        assert call(0, None, 5, C._ptr(q), 0, 1.0, C._ptr(one), None, None, None) == C.OK
        assert R.same(one[0], R.segment(np.zeros((0, 2), dtype), q, 1.0)[0])
        assert call(3, C._ptr(p), 5, C._ptr(q), 0, 3.0, C._ptr(one), None, None, None) == C.OK               # the rows are optional
        assert R.same(one[0], R.segment(p, q, 3.0)[0]) and one[0]["close_pairs"] == 15


class _NoLibrary:
    """Stands where a class keeps its handle: any use of it is a library call."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was touched: {name}")


@pytest.mark.parametrize("cls", CLASSES)
def test_python_checks_raise_before_any_library_call(nb, cls):
    e = object.__new__(getattr(nb, cls))
    e.h = _NoLibrary()
    e._n_worlds = 4
    try:
        bad_calls = [("limit2", dict(limit2=[1.0, 2.0, 3.0])), ("limit2", dict(limit2=[[1.0, 2.0, 3.0, 4.0]])), ("limit2", dict(limit2=1.0)),
                     ("limit2", dict(limit2=["a", "b", "c", "d"])), ("limit2", dict(limit2=[1j, 0, 0, 0])),
                     ("rows", dict(rows=1)), ("rows", dict(rows=None))]
        if cls in WITH_TRACERS:
            bad_calls += [("tracers", dict(tracers=1)), ("limit2", dict(limit2=[1.0], tracers=True))]
        for word, kw in bad_calls:
            with pytest.raises(ValueError, match=rf"{cls}\.encounters: .*{word}"):
                e.encounters(**kw)
        if cls not in WITH_TRACERS:
            with pytest.raises(TypeError):
                e.encounters(tracers=True)                                  # `tracers` exists only where the class has tracers
        for good in (dict(), dict(limit2=[np.nan, 0, np.inf, 1e300]), dict(limit2=np.arange(4), rows=False)):
            with pytest.raises(AssertionError, match="the library was touched: encounters"):
                e.encounters(**good)                                        # good arguments reach the handle
    finally:
        e.h = None
    z32, z64 = np.zeros((3, 2), np.float32), np.zeros((3, 2), np.float64)
    for bad in (dict(targets=np.zeros((3, 2), np.int32)), dict(targets=np.zeros((3, 3), np.float32)), dict(targets=np.zeros(3, np.float32)),
                dict(targets=z32, sources=z64), dict(targets=z64, sources=np.zeros((3, 3))), dict(targets=z64, limit2="1"),
                dict(targets=z64, limit2=None), dict(targets=z64, limit2=True)):
        with pytest.raises(ValueError, match="encounters_of"):
            nb.encounters_of(**bad)


def _check(nb, targets, sources, limit2, what):
    got, want = nb.encounters_of(targets, sources, limit2), R.segment(targets, sources, limit2)
    assert R.same_segment(got, want), (what, R.diff(got, want), got[0], want[0])
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", COUNTS)
def test_encounters_of_is_the_restatement_bit_for_bit_on_bodies(nb, dtype, n):
    seed = S.seed_of("host bodies", n, np.dtype(dtype).name)
    for k in range(3):                                                      # every kind of world of the scene
        pos = S.world(seed, k, n, dtype)
        for limit in S.limits(2, shift=k + n):
            rec = _check(nb, pos, None, dtype(limit), (k, n, limit))[0]
            assert rec["rows"] == rec["sources"] == n and rec["live_pairs"] + rec["skipped_pairs"] == n * max(n - 1, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n", [(m, 257) for m in COUNTS] + [(300, n) for n in COUNTS if n != 257])
def test_encounters_of_is_the_restatement_bit_for_bit_on_tracers(nb, dtype, m, n):
    seed = S.seed_of("host tracers", m, n, np.dtype(dtype).name)
    for k in range(3):
        bodies = S.world(seed, k, n, dtype)
        tr = S.tracers(seed, k, m, dtype, bodies)
        limit = S.limits(1, shift=k + m + n)[0]
        rec = _check(nb, tr, bodies, dtype(limit), (k, m, n, limit))[0]
        assert rec["rows"] == m and rec["sources"] == n and rec["live_pairs"] + rec["skipped_pairs"] == m * n


def _bits(v):
    return int(np.float64(v).view(np.uint64))


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_plant_behaves_as_the_scene_says(nb, dtype):
    n = 600
    seed = S.seed_of("plants", np.dtype(dtype).name)
    pos = S.world(seed, 0, n, dtype)
    at = S.planted(n, dtype)
    rec, idx, d2, close = nb.encounters_of(pos, None, 0.3)
    full = n * (n - 1)
    # rows holding NaN, +inf, -inf: no pair with them is live, in either direction; they are isolated
    dead = [at["nan"], at["pinf"], at["ninf"]]
    assert all(idx[r] == -1 and d2[r] == np.inf and close[r] == 0 for r in dead) and rec["isolated_rows"] == 3
    # the subnormal difference and the coincident pair are skipped, both ways: 2 * 3 * (n - 1) - 6 dead pairs and 4 more
    assert rec["skipped_pairs"] == 2 * 3 * (n - 1) - 6 + 4 and rec["live_pairs"] == full - rec["skipped_pairs"]
    assert idx[at["sub_a"]] != at["sub_b"] and idx[at["sub_b"]] != at["sub_a"]
    dx = pos[at["sub_b"], 0] - pos[at["sub_a"], 0]
    assert 0 < dx < np.finfo(dtype).tiny and pos[at["sub_a"], 0] == 0 and np.signbit(pos[at["sub_a"], 0])     # subnormal; the -0.0 row
    moved = pos.copy()
    moved[at["sub_b"], 0] = np.finfo(dtype).tiny                            # the smallest normal difference is a pair again
    assert nb.encounters_of(moved, None, 0.3)[0]["skipped_pairs"] == rec["skipped_pairs"] - 2
    # two coincident bodies beside a third: each one's neighbour is the third, not the other
    assert idx[at["coin_a"]] == idx[at["coin_b"]] == at["coin_third"] and d2[at["coin_a"]] == d2[at["coin_b"]] == 0.25
    assert idx[at["coin_third"]] == at["coin_a"] < at["coin_b"]             # a tie of two sources: the lower index
    assert close[at["coin_a"]] == close[at["coin_b"]] == 1 and close[at["coin_third"]] == 2      # 0.25 < 0.3
    assert all(nb.encounters_of(pos, None, 0.25)[3][[at["coin_a"], at["coin_b"], at["coin_third"]]] == 0)      # strict
    # a normal dx whose d2 underflows to +0: live, close under any positive limit, the world's minimum, at the lowest row
    step = pos[at["under_b"], 0] - pos[at["under_a"], 0]
    assert step >= np.finfo(dtype).tiny and step * step == 0
    assert idx[at["under_a"]] == at["under_b"] and idx[at["under_b"]] == at["under_a"]
    assert _bits(d2[at["under_a"]]) == 0 and close[at["under_a"]] >= 1
    assert (rec["min_row"], rec["min_source"], _bits(rec["min_d2"])) == (at["under_a"], at["under_b"], 0)
    tiny_limit = nb.encounters_of(pos, None, float(np.finfo(dtype).smallest_subnormal))
    assert tiny_limit[0]["close_pairs"] == 2 and tiny_limit[0]["close_rows"] == 2
    # every branch of the limit's comparison
    assert nb.encounters_of(pos, None, float("nan"))[0]["close_pairs"] == 0 == nb.encounters_of(pos, None, 0.0)[0]["close_pairs"]
    assert nb.encounters_of(pos, None, -1.0)[0]["close_pairs"] == 0
    assert nb.encounters_of(pos, None, float("inf"))[0]["close_pairs"] == rec["live_pairs"]       # (no d2 of this world overflows)
    # the farthest nearest neighbour
    has = idx >= 0
    assert rec["max_nn_d2"] == d2[has].max() and rec["max_nn_row"] == np.flatnonzero(has & (d2 == d2[has].max()))[0]
    # d2 overflows to +inf while sum is finite: a live pair, beside a world of one body, which has none
    two, one = S.world(seed, 2, 2, dtype), S.world(seed, 2, 1, dtype)
    rec2, idx2, d22, close2 = nb.encounters_of(two, None, float("inf"))
    assert list(idx2) == [1, 0] and list(d22) == [np.inf, np.inf] and list(close2) == [0, 0]      # inf < inf is false
    assert (rec2["live_pairs"], rec2["skipped_pairs"], rec2["isolated_rows"]) == (2, 0, 0)
    assert (rec2["min_row"], rec2["min_source"], rec2["min_d2"], rec2["max_nn_row"], rec2["max_nn_d2"]) == (0, 1, np.inf, 0, np.inf)
    rec1, idx1, d21, _ = nb.encounters_of(one, None, float("inf"))
    assert list(idx1) == [-1] and list(d21) == [np.inf] and (rec1["live_pairs"], rec1["skipped_pairs"], rec1["isolated_rows"]) == (0, 0, 1)
    assert (rec1["min_row"], rec1["min_source"], rec1["min_d2"], rec1["max_nn_row"], _bits(rec1["max_nn_d2"])) == (-1, -1, np.inf, -1, 0)
    # tracers: one on top of a body (that pair is skipped), one at NaN (isolated), one far outside (the farthest neighbour)
    m = 300
    tr = S.tracers(seed, 0, m, dtype, pos)
    ta = S.planted_tracers(m)
    trec, tidx, td2, _ = nb.encounters_of(tr, pos, 0.3)
    assert (tr[ta["on_body"]] == pos[n // 3]).all() and tidx[ta["on_body"]] not in (-1, n // 3)
    assert tidx[ta["nan"]] == -1 and trec["isolated_rows"] == 1 and trec["max_nn_row"] == ta["far"]
    assert trec["skipped_pairs"] == 3 * (m - 1) + n + 1 and trec["rows"] == m and trec["sources"] == n
    none = nb.encounters_of(np.zeros((0, 2), dtype), pos, 1.0)[0]           # a world without tracers
    assert (none["rows"], none["sources"], none["live_pairs"], none["skipped_pairs"], none["isolated_rows"]) == (0, n, 0, 0, 0)
    assert (none["min_row"], none["min_source"], none["min_d2"], none["max_nn_row"], _bits(none["max_nn_d2"])) == (-1, -1, np.inf, -1, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [64, 65, 257, R.CHUNK + 1])
def test_visibility_another_tie_rule_or_a_fused_d2_gives_other_bits_on_these_rows(nb, dtype, n):
    """Conditions on the inputs.  In the lattice world "the highest index of a tie" gives other nn_index than the contract's, for
    bodies and for tracers.  In the plain and the edge world a d2 computed as fma(dy, dy, dx*dx) changes at least one nn_d2 bit.
    In the lattice world it cannot: every coordinate is a small integer, every product and sum is exact, fused or not; there
    the two are asserted equal."""
    seed = S.seed_of("visibility", n, np.dtype(dtype).name)
    for k in range(3):
        pos = S.world(seed, k, n, dtype)
        tr = S.tracers(seed, k, n, dtype, pos)
        for targets, sources in ((pos, None), (tr, pos)):
            mine = nb.encounters_of(targets, sources, 1.5)
            assert R.same_segment(mine, R.segment(targets, sources, 1.5))
            fused = R.segment(targets, sources, 1.5, fused=True)
            highest = R.segment(targets, sources, 1.5, highest=True)
            if k % 3 == 1:
                assert R.same(fused[2], mine[2])                            # nothing to round
                assert not R.same(highest[1], mine[1]) and R.same(highest[2], mine[2])
                assert (highest[1] >= mine[1]).all()
            else:
                assert not R.same(fused[2], mine[2]), k
