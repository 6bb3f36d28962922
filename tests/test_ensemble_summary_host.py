"""Summaries of an ensemble (nbody_summary_*, the classes' summary(), nb.summary_of) without a GPU: the ten declared names in both
libraries and in the binding, no other name under the prefix, the ABI version, the record's size and offsets from a C99 program,
NULL-handle calls, the Python checks, nbody_summary_of_f32 / _of_f64 against the NumPy restatement of the contract
(tests/_summary_restatement.py) on the scene of tests/_summary_scene.py, what every planted row is there for, and the visibility
condition: on these very rows another order of additions gives other bits, so the GPU tests can see the order."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _summary_restatement as R
import _summary_scene as S

HANDLES = ("ensemble", "ensemble64", "ragged", "ragged64", "restricted", "restricted64", "rr", "rr64")
CALLS = ["nbody_summary_" + s for s in HANDLES]
NAMES = CALLS + ["nbody_summary_of_f32", "nbody_summary_of_f64"]
CLASSES = ["Ensemble", "Ensemble64", "RaggedEnsemble", "RaggedEnsemble64", "RestrictedEnsemble", "RestrictedEnsemble64",
           "RaggedRestrictedEnsemble", "RaggedRestrictedEnsemble64"]
WITH_TRACERS = {"RestrictedEnsemble", "RestrictedEnsemble64", "RaggedRestrictedEnsemble", "RaggedRestrictedEnsemble64"}
ROWS = [0, 1, 2, 255, 256, 257, 600, 4096, 4097, 8192, 9000]
H = S.HEIGHT


def test_header_declares_the_summary_calls_and_both_libraries_export_them(nb):
    C = nb._capi
    assert len(NAMES) == 10
    declared = C.declared_symbols()
    assert sorted(s for s in declared if s.startswith("nbody_summary_")) == sorted(NAMES)      # these and no other
    assert sorted(s for s in C._SIGS if s.startswith("nbody_summary_")) == sorted(NAMES)
    assert sorted(C._SIGS) == declared
    for path in (C.LIB_PATH, C.LAB_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in NAMES if not hasattr(lib, s)], path
        exported = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert sorted(set(re.findall(r"\bnbody_summary_\w+", exported))) == sorted(NAMES), path
    with open(C.HEADER_PATH) as f:
        head = f.read()
    assert int(re.search(r"#define\s+NBODY_ABI_VERSION\s+(\d+)", head).group(1)) == 3 == C.ABI_VERSION    # new symbols only
    assert "nbody_summary" not in head                                      # declared in nbody_ensemble.h, which it includes
    with open(os.path.join(os.path.dirname(C.HEADER_PATH), "nbody_ensemble.h")) as f:
        ens = f.read()
    note = r"\s*(/\*.*?\*/)?\s*"
    for name in CALLS:
        handle = "nbody_" + name[len("nbody_summary_"):]
        assert re.search(rf"int\s+{name}\s*\(\s*{handle}\s*\*\s*e,\s*uint32_t\s+flags,\s*uint32_t\s+height,\s*const\s+int32_t\s*\*\s*ref{note},"
                         rf"\s*nbody_world_summary\s*\*\s*out{note}\)\s*;", ens), name
        assert len(C._SIGS[name][1]) == 5
    for name, real in (("nbody_summary_of_f32", "float"), ("nbody_summary_of_f64", "double")):
        assert re.search(rf"int\s+{name}\s*\(\s*int64_t\s+rows,\s*const\s+{real}\s*\*\s*pos_xy,\s*const\s+{real}\s*\*\s*vel_xy,\s*"
                         rf"const\s+uint32_t\s*\*\s*weight{note},\s*const\s+{real}\s*\*\s*ref_pos_xy{note},\s*const\s+{real}\s*\*\s*ref_vel_xy,\s*"
                         rf"uint32_t\s+height,\s*nbody_world_summary\s*\*\s*out\s*\)\s*;", ens), name
        assert len(C._SIGS[name][1]) == 8
    assert re.search(r"#define\s+NBODY_SUMMARY_TRACERS\s+1u", ens) and C.SUMMARY_TRACERS == 1
    # the prefix is its own: it is a prefix of no other set of names and none is a prefix of it
    others = ("nbody_ensemble_", "nbody_ensemble64_", "nbody_ragged_", "nbody_ragged64_", "nbody_restricted_", "nbody_restricted64_",
              "nbody_rr_", "nbody_rr64_", "nbody_frames_", "nbody_deltas_", "nbody_delta_", "nbody_sweep_")
    assert not [s for s in NAMES if s.startswith(others)]
    assert not [s for s in declared if s.startswith("nbody_summary") and s not in NAMES]
    # what the header says is not offered
    for words in ("phase-space separation", "potential energy", "device-pointer variant", "nbody_ctx contexts"):
        assert words in ens[ens.index("summaries of an ensemble"):], words
    assert "summary_of" in nb.__all__ and nb.summary_of is nb.ensemble.summary_of and nb.SUMMARY_DTYPE is C.SUMMARY_DTYPE
    for cls in CLASSES:
        assert callable(getattr(nb, cls).summary), cls


def test_the_record_is_136_bytes_with_the_dtypes_offsets_in_c99(nb, tmp_path):
    C = nb._capi
    fields = list(nb.SUMMARY_DTYPE.names)
    assert fields == ["rows", "counted", "in_bounds", "sep_rows", "mass", "min_x", "min_y", "max_x", "max_y", "max_speed2", "sum_wx",
                      "sum_wy", "sum_wvx", "sum_wvy", "sum_wv2", "sep_max2", "sep_sum2"]
    assert nb.SUMMARY_DTYPE.itemsize == 136 == R.DTYPE.itemsize
    assert [nb.SUMMARY_DTYPE.fields[f][1] for f in fields] == [8 * i for i in range(17)] == [R.DTYPE.fields[f][1] for f in fields]
    assert [nb.SUMMARY_DTYPE.fields[f][0] for f in fields] == [np.dtype(np.int64)] * 4 + [np.dtype(np.float64)] * 13
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nbody_hip.h"\nint main(void) {\n'
                   '  printf("%u", (unsigned)sizeof(nbody_world_summary));\n' +
                   "".join(f'  printf(" %u", (unsigned)offsetof(nbody_world_summary, {f}));\n' for f in fields) +
                   '  printf(" %u\\n", (unsigned)NBODY_SUMMARY_TRACERS);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    inc = os.path.dirname(C.HEADER_PATH)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", inc, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [136] + [8 * i for i in range(17)] + [1]


@pytest.mark.parametrize("which", ["product", "lab"])
def test_null_handle_calls_and_what_summary_of_refuses(nb, which):
    C = nb._capi
    lib = C._load(which)
    out = np.zeros(4, nb.SUMMARY_DTYPE)
    out["rows"] = 7
    ref = np.zeros(4, np.int32)
    for name in CALLS:
        for flags in (0, 1, 2):
            assert getattr(lib, name)(None, flags, 100, ref.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), C._ptr(out)) == C.ERR_INVALID, name
        assert getattr(lib, name)(None, 0, 0, None, None) == C.ERR_INVALID, name
    for name, dtype in (("nbody_summary_of_f32", np.float32), ("nbody_summary_of_f64", np.float64)):
        call = getattr(lib, name)
        p, v = np.ones((3, 2), dtype), np.ones((3, 2), dtype)
        assert call(-1, C._ptr(p), C._ptr(v), None, None, None, 0, C._ptr(out)) == C.ERR_INVALID
        assert call(3, C._ptr(p), C._ptr(v), None, None, None, 0, None) == C.ERR_INVALID
        assert call(3, None, C._ptr(v), None, None, None, 0, C._ptr(out)) == C.ERR_INVALID
        assert call(3, C._ptr(p), None, None, None, None, 0, C._ptr(out)) == C.ERR_INVALID
        assert call(3, C._ptr(p), C._ptr(v), None, C._ptr(p), None, 0, C._ptr(out)) == C.ERR_INVALID   # a reference without velocities
        assert (out["rows"] == 7).all() and not out["mass"].any()
        one = np.zeros(1, nb.SUMMARY_DTYPE)
        assert call(0, None, None, None, None, None, 5, C._ptr(one)) == C.OK                          # no rows need no arrays
        assert R.same(one[0], R.record(np.zeros((0, 2), dtype), np.zeros((0, 2), dtype), None, None, 5))
        assert call(3, C._ptr(p), C._ptr(v), None, C._ptr(p), C._ptr(v), 2, C._ptr(one)) == C.OK
        assert R.same(one[0], R.record(p, v, None, (p, v), 2))


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
        bad_calls = [
            ("height", dict(height=-1)), ("height", dict(height=(1 << 24) + 1)), ("height", dict(height=1.5)), ("height", dict(height=True)),
            ("ref", dict(ref=[0, 1, 2])), ("ref", dict(ref=[[0, 1, 2, 3]])), ("ref", dict(ref=[0.0, 1.0, 2.0, 3.0])),
            (r"ref\[2\] = 4 of world 2", dict(ref=[0, 1, 4, 3])), (r"ref\[1\] = -2 of world 1", dict(ref=[0, -2, 1, 3])),
        ]
        for word, kw in bad_calls:
            with pytest.raises(ValueError, match=rf"{cls}\.summary: .*{word}"):
                e.summary(**kw)
        if cls in WITH_TRACERS:
            with pytest.raises(ValueError, match="height"):
                e.summary(height=-1, tracers=True)
        else:
            with pytest.raises(TypeError):
                e.summary(tracers=True)                                     # `tracers` exists only where the class has tracers
        with pytest.raises(AssertionError, match="the library was touched: summary"):
            e.summary(height=1 << 24, ref=[-1, 0, 3, 3])                    # good arguments reach the handle
    finally:
        e.h = None
    for bad in (dict(pos=np.zeros((3, 2), np.int32), vel=np.zeros((3, 2), np.int32)), dict(pos=np.zeros((3, 3), np.float32), vel=np.zeros((3, 3), np.float32)),
                dict(pos=np.zeros((3, 2), np.float32), vel=np.zeros((3, 2), np.float64)), dict(pos=np.zeros((3, 2), np.float32), vel=np.zeros((2, 2), np.float32)),
                dict(pos=np.zeros((3, 2), np.float64), vel=np.zeros((3, 2), np.float64), weight=np.ones(3)),
                dict(pos=np.zeros((3, 2), np.float64), vel=np.zeros((3, 2), np.float64), ref=np.zeros((3, 2))),
                dict(pos=np.zeros((3, 2), np.float64), vel=np.zeros((3, 2), np.float64), height=-1)):
        with pytest.raises(ValueError, match="summary_of"):
            nb.summary_of(**bad)


def _segments(dtype, rows, k=0):
    """World k's bodies and its tracers at `rows` rows, each with the rows of world k + 1 as the reference."""
    for tracers in (False, True):
        pos, vel, w = S.segment(S.seed_of(rows, dtype, tracers), k, rows, dtype, tracers)
        rp, rv, _ = S.segment(S.seed_of(rows, dtype, tracers), k + 1, rows, dtype, tracers)
        yield tracers, pos, vel, (None if tracers else w), (rp, rv)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("rows", ROWS)
def test_summary_of_is_the_restatement_bit_for_bit(nb, dtype, rows):
    for k in range(4):                                                      # every kind of world of the scene
        for tracers, pos, vel, w, ref in _segments(dtype, rows, k):
            for r in (None, ref, (pos, vel)):
                got, want = nb.summary_of(pos, vel, w, r, H), R.record(pos, vel, w, r, H)
                assert R.same(got, want), (k, tracers, r is not None, R.diff(got, want), got, want)
                x, y = pos[:, 0].astype(np.float64), pos[:, 1].astype(np.float64)
                inside = sum(1 for a, b in zip(x, y) if b < H and a < H and b >= 0 and a >= 0)     # the predicate, written out
                assert got["in_bounds"] == inside and got["rows"] == rows
                assert nb.summary_of(pos, vel, w, r, 0)["in_bounds"] == 0
                fin = np.isfinite(pos).all(axis=1) & np.isfinite(vel).all(axis=1)
                whole = w if w is not None else np.ones(rows, np.uint32)
                held = whole.astype(np.float32).astype(np.float64) if dtype == np.float32 else whole
                assert got["counted"] == fin.sum() and got["mass"] == float(sum(int(v) for v in held[fin]))   # the integer sum
                if r is None:
                    assert got["sep_rows"] == 0 and _bits(got["sep_max2"]) == 0 and _bits(got["sep_sum2"]) == 0
                elif r[0] is pos:
                    assert got["sep_rows"] == got["counted"] and _bits(got["sep_max2"]) == 0 and _bits(got["sep_sum2"]) == 0


def _bits(v):
    return int(np.float64(v).view(np.uint64))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_planted_row_behaves_as_the_scene_says(nb, dtype):
    rows = 600
    for tracers in (False, True):
        seed = S.seed_of(rows, dtype, tracers)
        w_of = lambda w: None if tracers else w  # noqa: E731
        # a plain world: every special row is left out of `counted`
        pos, vel, w = S.segment(seed, 0, rows, dtype, tracers)
        at = S.planted(seed, 0, rows, dtype, tracers)
        full = nb.summary_of(pos, vel, w_of(w), None, H)
        special = [at[f"{s}_{c}"] for s in ("nan", "pinf", "ninf") for c in ("x", "y", "vx", "vy")] + [at["inside_nan_v"]]
        assert len(set(special)) == 13 and full["counted"] == rows - 13
        for name in ["inside_nan_v"] + [f"{s}_{c}" for s in ("nan", "pinf", "ninf") for c in ("x", "y", "vx", "vy")]:
            # the row keeps its slot (it adds nothing there): replaced by another uncounted row the record is the same
            p2, v2 = pos.copy(), vel.copy()
            p2[at[name]], v2[at[name]] = (np.nan, np.nan), (np.nan, np.nan)
            less = nb.summary_of(p2, v2, w_of(w), None, H)
            inside = name == "inside_nan_v" or (name.endswith(("vx", "vy")) and _inside(pos[at[name]]))
            assert less["in_bounds"] == full["in_bounds"] - (1 if inside else 0), name
            for f in R.DTYPE.names:
                if f != "in_bounds":
                    assert R.same(R.only(less, f), R.only(full, f)), (name, f)
        assert _inside(pos[at["inside_nan_v"]]) and _inside(pos[at["edge_in"]]) and not _inside(pos[at["edge_out"]])
        p2 = pos.copy()
        p2[at["edge_out"]] = p2[at["edge_in"]]                              # exactly H is outside, the float below it inside
        assert nb.summary_of(p2, vel, w_of(w), None, H)["in_bounds"] == full["in_bounds"] + 1
        if not tracers:
            for name, value, held32 in (("w10", 10, 10.0), ("w11", 11, 11.0), ("w2p24", (1 << 24) + 1, 2.0 ** 24), ("wmax", (1 << 32) - 1, 2.0 ** 32)):
                assert w[at[name]] == value
                w2 = w.copy()
                w2[at[name]] = 1
                held = held32 if dtype == np.float32 else float(value)      # f32 handles hold `weight as f32`
                assert full["mass"] - nb.summary_of(pos, vel, w2, None, H)["mass"] == held - 1.0, name
        # the "zeros" world: the zeros are the extreme values and their signs decide
        pos, vel, w = S.segment(seed, 1, rows, dtype, tracers)
        z = nb.summary_of(pos, vel, w_of(w), None, H)
        assert _bits(z["max_x"]) == _bits(0.0) and _bits(z["min_y"]) == _bits(-0.0)
        assert z["min_x"] < 0 and z["max_y"] > 0
        flipped = pos.copy()
        flipped[pos == 0] = -pos[pos == 0]
        z2 = nb.summary_of(flipped, vel, w_of(w), None, H)
        assert _bits(z2["max_x"]) == _bits(0.0) and _bits(z2["min_y"]) == _bits(-0.0)     # order-free: the same zeros in other rows
        only = pos.copy()
        only[S.planted(seed, 1, rows, dtype, tracers)["zero_b"]] = (-0.0, 0.0)            # no +0.0 in x, no -0.0 in y any more
        z3 = nb.summary_of(only, vel, w_of(w), None, H)
        assert _bits(z3["max_x"]) == _bits(-0.0) and _bits(z3["min_y"]) == _bits(0.0)
        # the "huge" world, float64 only: the square overflows, the sum is +inf, nothing is NaN
        pos, vel, w = S.segment(seed, 2, rows, dtype, tracers)
        g = nb.summary_of(pos, vel, w_of(w), None, H)
        if dtype == np.float64:
            assert g["sum_wv2"] == np.inf and g["max_speed2"] == np.inf and np.isfinite(g["sum_wvx"]) and np.isfinite(g["sum_wvy"])
        else:
            assert np.isfinite(g["sum_wv2"]) and np.isfinite(g["max_speed2"])
    # nothing counted: the empty extremes
    nanp = np.full((5, 2), np.nan, dtype)
    e = nb.summary_of(nanp, nanp, None, (nanp, nanp), H)
    assert e["rows"] == 5 and e["counted"] == 0 and e["sep_rows"] == 0 and e["in_bounds"] == 0
    assert (e["min_x"], e["min_y"], e["max_x"], e["max_y"]) == (np.inf, np.inf, -np.inf, -np.inf)
    assert all(_bits(e[f]) == 0 for f in ("mass", "max_speed2", "sep_max2") + R.ORDERED)


def _inside(p):
    x, y = float(p[0]), float(p[1])
    return y < H and x < H and y >= 0 and x >= 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("rows,tracers", [(600, False), (4096, False), (4097, True), (9000, True)])
def test_visibility_another_order_gives_other_bits_on_these_rows(nb, dtype, rows, tracers):
    """A condition on the inputs: in world 0 of the scene, measured from world 1, each of the six ordered sums is finite and the
    contract's value differs from an ascending-row sequential sum, from a 64-chain version and — with three chunks, at 9000 rows —
    from chunks combined by a stride tree, (c0 + c2) + c1.  At 4097 rows there are two chunks and any way to combine two values is
    c0 + c1 (IEEE addition commutes): no order of the chunks can be seen there, and that is asserted instead."""
    (_, pos, vel, w, ref), = [s for s in _segments(dtype, rows) if s[0] == tracers]
    got = nb.summary_of(pos, vel, w, ref, H)
    t = R.terms(pos, vel, w, ref)[2]
    for f in R.ORDERED:
        mine = R.ordered_sum(t[f])
        assert np.isfinite(mine) and _bits(mine) == _bits(got[f]), f
        assert _bits(R.ordered_sum(t[f], sequential=True)) != _bits(mine), (f, "sequential")
        assert _bits(R.ordered_sum(t[f], chains=64)) != _bits(mine), (f, "64 chains")
        if rows > 2 * R.CHUNK:
            assert _bits(R.ordered_sum(t[f], chunk_tree=True)) != _bits(mine), (f, "chunk tree")
        elif rows > R.CHUNK:
            assert _bits(R.ordered_sum(t[f], chunk_tree=True)) == _bits(mine), (f, "two chunks")
