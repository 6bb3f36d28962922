"""Ensembles: many small worlds of one size, stepped together (nbody_ensemble_*, include/nbody_hip.h).

The same scene under many seeds, a sweep over initial conditions, many independent clusters: below a few thousand bodies one
world cannot fill the device, and one `World` per world costs one launch chain per world and step.  An `Ensemble` holds B worlds
of n bodies each (n <= 4096) on the device and steps all of them with one launch per step; every world takes the step of
`World(method="direct")`, independently of the others — EXACT bit-identical to the oracle's update_direct of that world alone,
FAST within the tolerance of DESIGN.md, AUTO choosing between them per world and per step on the device.

`Ensemble` is float32 and takes float32 arrays only; `Ensemble64` (nbody_ensemble64_*) is its double-precision sibling with the
same constructor and methods, float64 arrays only: every world takes the step of an f64 `World(method="direct")` — EXACT and AUTO
bit-identical to the oracle's update_direct on float64, FAST (opt-in, per world and per step on the device) within 1e-12 of
sum |term|.  Shapes, dtypes and the size limits are checked here, with ValueError, before a handle exists.

`RaggedEnsemble` (nbody_ragged_*) holds float32 worlds of DIFFERENT sizes — a sweep over N, clusters drawn from a mass function,
halos cut out of a larger run — and steps them together with at most six launches per step (`ragged_plan` shows which).  Every
world takes the same step: EXACT bit-identical to the oracle of that world alone, FAST bit-identical to an `Ensemble` holding
that world alone, AUTO per world and per step on the device.  `RaggedEnsemble64` (nbody_ragged64_*) is its double-precision
sibling, float64 arrays only: EXACT and AUTO bit-identical to the oracle's update_direct of that world alone on float64, FAST
(opt-in) bit-identical to an `Ensemble64` holding that world alone.

`RestrictedEnsemble` (nbody_restricted_*) is an `Ensemble` whose worlds carry m tracers each — massless points that feel their
own world's bodies and nothing else: the restricted problem under many seeds.  The bodies are bit-identical to an `Ensemble` of
the same worlds; a tracer is EXACT bit-identical to the oracle's direct_accel at it + Euler, FAST within the tolerance of
DESIGN.md, AUTO per world and per step on the device with a per-tracer exception for a tracer outside FAST's domain.
`RestrictedEnsemble64` (nbody_restricted64_*) is its double-precision sibling, float64 arrays only: the bodies are bit-identical
to an `Ensemble64` of the same worlds; a tracer is EXACT (and AUTO) bit-identical to the oracle's direct_accel at it + Euler on
float64, FAST (opt-in, per world and per step on the device, with the same per-tracer exception) within 1e-12 of sum |term|.

`RaggedRestrictedEnsemble` (nbody_rr_*) holds float32 worlds of DIFFERENT sizes, each with a tracer count of its own — a stability
map over systems with different numbers of massive bodies, halos with their own tracer populations — and steps them together
with at most twelve launches per step (`ragged_plan` shows the bodies', `rr_plan` the tracers').  The bodies are bit-identical
to a `RaggedEnsemble` of the same worlds; a tracer is EXACT bit-identical to the oracle, FAST bit-identical to a
`RestrictedEnsemble` holding its world alone.

Every class has `frames(height, render_px)` (nbody_frames_*): the reference's draw() raster of every world's own rows from one
call, uint8 [B, render_px, render_px, 4] — the classes with tracers take `tracers=True` to paint them after their world's
bodies — and `contact_sheet(frames)` tiles such frames into one image on the host.

Every class has `deltas()` (nbody_deltas_*) too: one lossless NBD1 delta stream per world from one call, byte for byte what a
`World` holding that world alone hands out through delta_begin / delta_end — the classes with tracers take `tracers=True` for
the tracers' sequence — and `DeltasDecoder(n_worlds)` is the receiving side, one `DeltaDecoder` per world.  Snapshots of an
ensemble are not offered: `particles()` hands the rows out whole.

Every class has `sweep(delta, clamp=None, steps=None)` (nbody_sweep_*): an update in which world k steps by delta[k] under
clamp[k] and takes steps[k] steps, then stands still bit for bit — a time-step convergence study or a softening sweep in one
handle.  World k's bits are those of the same class holding world k alone with that clamp, stepped by update(delta[k],
n_steps=steps[k]).

Every class has `summary(height=0, ref=None)` (nbody_summary_*) as well: one record per world — rows, finite rows, rows inside the
frame, mass, extent, largest squared speed, the weighted sums behind centre of mass, momentum and kinetic sum, and the squared
separations from the world ref[k] names — as an array of `SUMMARY_DTYPE`, computed on the device from the current rows, every
field a stated function of the world's own rows bit for bit; the classes with tracers take `tracers=True` for the
tracers' segments.  `summary_of(pos, vel, weight, ref, height)` is the same contract in host code, for one segment.

Every class has `encounters(limit2=None)` (nbody_encounters_*) too, the quadratic sibling of `summary`: per body its nearest
neighbour (`nn_index`, `nn_d2`) and the number of its pairs closer than limit2[k] (`close`), and per world a record of
`ENCOUNTERS_DTYPE` — live, skipped and close pairs, the closest pair, the most isolated body — in the handle's own precision with
the step's own expressions, so with limit2=None `close_pairs` counts the ordered pairs whose force the clamp altered.  Every
output is order-free, hence bit for bit; the classes with tracers take `tracers=True` for every tracer's nearest
body.  `encounters_of(targets, sources, limit2)` is the same contract in host code, for one segment.

Every class has `watch(delta, n_steps, limit2=None, height=0, stride=1)` (nbody_watch_*): an update that the device samples
before, between and after its steps — per body its closest approach over the run and the sample it occurred at, the first sample
with a pair closer than limit2[k] and how many samples had one, the first sample outside the frame — and per world a record of
`WATCH_DTYPE`, without a host synchronisation between the steps; the rows afterwards are those of `update`.  The classes with
tracers take `tracers=True` for every tracer against its world's bodies.  `watch_merge(first, second, steps_before)` joins a call
and the `resume=True` call that continued it into what one call gives, bit for bit.

Every class has `watch_sweep(delta, clamp=None, steps=None, n_steps=None, stride=1, limit2=None, height=0)` (nbody_wsweep_*): the
two together, a `sweep` watched on every world's own schedule — world k is sampled at the s <= steps[k] with s % stride[k] == 0,
against its own clamp[k] where limit2 is None — with world k's record and rows bit for bit those of `watch` on the same class
holding world k alone, and the rows afterwards those of `sweep`.  `watch_sweep_plan(steps, n_steps, stride, resume)` gives the
samples per world and the number of sampling launches of a schedule in host code.

The four classes without tracers — `Ensemble`, `Ensemble64`, `RaggedEnsemble`, `RaggedEnsemble64` — have `run(delta, n_steps=None,
clamp=None, steps=None)` (nbody_resident_*): `sweep` as a resident run, for worlds of at most 256 bodies.  One block per world
keeps the world in LDS and takes up to 1024 of its steps per launch; the rows afterwards are bit for bit those of `sweep`.
`resident_plan(sizes, steps, n_steps, dtype)` gives the launches of such a call and their LDS in host code.
"""
from __future__ import annotations

import numpy as np

from . import _capi
from ._capi import Counting

MAX_BODIES = 4096          # per world: its sources stage whole in LDS
MAX_ROWS = 1 << 26         # worlds * bodies

_ARITH = {"auto": _capi.ARITH_AUTO, "fast": _capi.ARITH_FAST, "exact": _capi.ARITH_EXACT}


def _streams(handle, tracers, key):
    """handle.deltas(...) cut into one bytes object per world."""
    buf, off, step = handle.deltas(tracers, key)
    return [buf[int(off[k]):int(off[k + 1])].tobytes() for k in range(off.shape[0] - 1)], step


def _checked_sweep(who, b, dtype, delta, clamp, steps, n_steps, what="sweep"):
    """The arguments of `sweep` for b worlds -> (delta dtype[b], clamp float32[b] or None, steps int32[b] or None, n_steps),
    contiguous; ValueError naming `who` and the argument for anything else.  n_steps defaults to max(steps), or 1 without steps."""
    def per_world(name, a, to):
        a = np.asarray(a)
        if a.ndim != 1 or a.shape[0] != b:
            raise ValueError(f"{who}.{what}: {name} must hold one value per world ({b} worlds), got shape {a.shape}")
        if a.dtype.kind not in "fiu":
            raise ValueError(f"{who}.{what}: {name} must be numbers, got {a.dtype}")
        return a if to is None else np.ascontiguousarray(a, dtype=to)
    if delta is None:
        raise ValueError(f"{who}.{what}: delta is required, one time step per world")
    delta = per_world("delta", delta, dtype)
    if clamp is not None:
        clamp = per_world("clamp", clamp, np.float32)
    if n_steps is not None:
        if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or not 0 <= int(n_steps) < 1 << 31:
            raise ValueError(f"{who}.{what}: n_steps must be an integer 0 .. 2^31 - 1, got {n_steps!r}")
        n_steps = int(n_steps)
    if steps is not None:
        steps = per_world("steps", steps, None)
        if steps.dtype.kind == "f":
            if not (np.isfinite(steps).all() and (steps == np.floor(steps)).all()):
                raise ValueError(f"{who}.{what}: steps must be whole numbers")
        top = int(steps.max()) if n_steps is None else n_steps
        if top >= 1 << 31:
            raise ValueError(f"{who}.{what}: steps must be below 2^31")
        bad = np.flatnonzero((steps < 0) | (steps > top))
        if bad.size:
            k = int(bad[0])
            raise ValueError(f"{who}.{what}: steps[{k}] = {steps[k]} of world {k} is outside 0 .. n_steps = {top}")
        steps, n_steps = np.ascontiguousarray(steps, dtype=np.int32), top
    return delta, clamp, steps, 1 if n_steps is None else n_steps


SUMMARY_DTYPE = _capi.SUMMARY_DTYPE
MAX_HEIGHT = 1 << 24       # of a summary's frame, as the frames'


def _checked_summary(who, b, height, ref):
    """The arguments of `summary` for b worlds -> (height, ref int32[b] contiguous or None); ValueError naming `who` and the
    argument for anything else."""
    if isinstance(height, bool) or not isinstance(height, (int, np.integer)) or not 0 <= int(height) <= MAX_HEIGHT:
        raise ValueError(f"{who}.summary: height must be an integer 0 .. 2^24, got {height!r}")
    if ref is not None:
        ref = np.asarray(ref)
        if ref.ndim != 1 or ref.shape[0] != b:
            raise ValueError(f"{who}.summary: ref must hold one world index per world ({b} worlds), got shape {ref.shape}")
        if ref.dtype.kind not in "iu":
            raise ValueError(f"{who}.summary: ref must be integers (-1: no reference), got {ref.dtype}")
        bad = np.flatnonzero((ref < -1) | (ref >= b))
        if bad.size:
            k = int(bad[0])
            raise ValueError(f"{who}.summary: ref[{k}] = {ref[k]} of world {k} is outside -1 .. {b - 1}")
        ref = np.ascontiguousarray(ref, dtype=np.int32)
    return int(height), ref


def summary_of(pos, vel, weight=None, ref=None, height=0):
    """One segment's summary record in host code (nbody_summary_of_f32 / _of_f64 by the arrays' dtype; no GPU needed): pos, vel
    [rows, 2] float32 or float64, weight [rows] integers or None (all 1), ref None or a pair (position[rows, 2], velocity[rows, 2])
    of the reference world's rows -> a `SUMMARY_DTYPE` scalar, the bits `summary()` gives for a world holding these rows."""
    pos, vel = np.asarray(pos), np.asarray(vel)
    if pos.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"summary_of: pos must be float32 or float64, got {pos.dtype}")
    if pos.ndim != 2 or pos.shape[1] != 2:
        raise ValueError(f"summary_of: pos must be [rows, 2], got {pos.shape}")
    rows = pos.shape[0]

    def same(name, a):
        a = np.asarray(a)
        if a.dtype != pos.dtype or a.shape != pos.shape:
            raise ValueError(f"summary_of: {name} must be {pos.dtype} {pos.shape} as pos is, got {a.dtype} {a.shape}")
        return np.ascontiguousarray(a)
    pos, vel = np.ascontiguousarray(pos), same("vel", vel)
    if weight is not None:
        weight = np.asarray(weight)
        if weight.shape != (rows,) or weight.dtype.kind not in "ui":
            raise ValueError(f"summary_of: weight must be integers [rows] = {(rows,)}, got {weight.dtype} {weight.shape}")
        weight = np.ascontiguousarray(weight, dtype=np.uint32)
    rp = rv = None
    if ref is not None:
        if not isinstance(ref, (tuple, list)) or len(ref) != 2:
            raise ValueError("summary_of: ref must be None or a pair (position[rows, 2], velocity[rows, 2])")
        rp, rv = same("ref position", ref[0]), same("ref velocity", ref[1])
    height, _ = _checked_summary("summary_of", 0, height, None)
    out = np.zeros(1, SUMMARY_DTYPE)
    call = getattr(_capi.load(), "nbody_summary_of_f32" if pos.dtype == np.float32 else "nbody_summary_of_f64")
    rc = call(rows, _capi._ptr(pos), _capi._ptr(vel), _capi._ptr(weight), _capi._ptr(rp), _capi._ptr(rv), height, _capi._ptr(out))
    if rc != _capi.OK:
        raise _capi.NBodyError(rc, "summary_of: refused")
    return out[0]


class _Summary:
    """`summary` for the ensemble classes without tracers: the class keeps `_n_worlds`, its handle has `summary`."""

    def summary(self, height=0, ref=None):
        """-> SUMMARY_DTYPE[B]: one record per world of its bodies' current rows (nbody_summary_*), bit for bit `summary_of` of
        that world's rows.  height: the frame of `in_bounds` (0: none).  ref: None, or one world index per world (-1: none) — the
        world whose rows sep_rows, sep_max2 and sep_sum2 are measured from.  The arguments are checked here, with ValueError,
        before the library is touched; the state is untouched."""
        height, ref = _checked_summary(type(self).__name__, self._n_worlds, height, ref)
        return self.h.summary(height, ref)


class _SummaryWithTracers:
    """`summary` for the ensemble classes with tracers."""

    def summary(self, height=0, ref=None, tracers=False):
        """-> SUMMARY_DTYPE[B]: one record per world of its bodies' current rows or, with tracers=True, of its tracers' (w = 1; a
        world without tracers: rows == 0), bit for bit `summary_of` of those rows.  height: the frame of `in_bounds` (0: none).
        ref: None, or one world index per world (-1: none).  The arguments are checked here, with ValueError, before the library
        is touched; the state is untouched."""
        height, ref = _checked_summary(type(self).__name__, self._n_worlds, height, ref)
        return self.h.summary(height, ref, bool(tracers))


ENCOUNTERS_DTYPE = _capi.ENCOUNTERS_DTYPE


def _checked_encounters(who, b, limit2, tracers, rows):
    """The arguments of `encounters` for b worlds -> (limit2 float32[b] contiguous or None, tracers, rows); ValueError naming
    `who` and the argument for anything else.  NaN and infinite limits are values like any other."""
    if limit2 is not None:
        limit2 = np.asarray(limit2)
        if limit2.ndim != 1 or limit2.shape[0] != b:
            raise ValueError(f"{who}.encounters: limit2 must hold one squared distance per world ({b} worlds), got shape {limit2.shape}")
        if limit2.dtype.kind not in "fiu":
            raise ValueError(f"{who}.encounters: limit2 must be real numbers, got {limit2.dtype}")
        with np.errstate(over="ignore"):
            limit2 = np.ascontiguousarray(limit2, dtype=np.float32)
    for name, flag in (("tracers", tracers), ("rows", rows)):
        if not isinstance(flag, (bool, np.bool_)):
            raise ValueError(f"{who}.encounters: {name} must be True or False, got {flag!r}")
    return limit2, bool(tracers), bool(rows)


def encounters_of(targets, sources=None, limit2=0.001):
    """One segment's encounters in host code (nbody_encounters_of_f32 / _of_f64 by the arrays' dtype; no GPU needed): targets
    [rows, 2] float32 or float64; sources None — the targets are a world's bodies, each measured against the others — or
    [n, 2] of the same dtype, a world's bodies around these tracers; limit2 a number, in the arrays' precision -> (record,
    nn_index int32[rows], nn_d2 [rows], close uint32[rows]): the `ENCOUNTERS_DTYPE` scalar and the rows `encounters()` gives for a
    world holding these rows."""
    targets = np.asarray(targets)
    if targets.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"encounters_of: targets must be float32 or float64, got {targets.dtype}")
    if targets.ndim != 2 or targets.shape[1] != 2:
        raise ValueError(f"encounters_of: targets must be [rows, 2], got {targets.shape}")
    targets = np.ascontiguousarray(targets)
    own = sources is None
    if own:
        sources = targets
    else:
        sources = np.asarray(sources)
        if sources.dtype != targets.dtype or sources.ndim != 2 or sources.shape[1] != 2:
            raise ValueError(f"encounters_of: sources must be {targets.dtype} [n, 2] as targets are, got {sources.dtype} {sources.shape}")
        sources = np.ascontiguousarray(sources)
    if isinstance(limit2, (bool, np.bool_)) or not isinstance(limit2, (int, float, np.integer, np.floating)):
        raise ValueError(f"encounters_of: limit2 must be a number, got {limit2!r}")
    rows = targets.shape[0]
    out = np.zeros(1, ENCOUNTERS_DTYPE)
    index, d2, close = np.zeros(rows, np.int32), np.zeros(rows, targets.dtype), np.zeros(rows, np.uint32)
    call = getattr(_capi.load(), "nbody_encounters_of_f32" if targets.dtype == np.float32 else "nbody_encounters_of_f64")
    with np.errstate(over="ignore"):
        limit2 = float(targets.dtype.type(limit2))
    rc = call(rows, _capi._ptr(targets), sources.shape[0], _capi._ptr(sources), 1 if own else 0, limit2, _capi._ptr(out),
              _capi._ptr(index), _capi._ptr(d2), _capi._ptr(close))
    if rc != _capi.OK:
        raise _capi.NBodyError(rc, "encounters_of: refused")
    return out[0], index, d2, close


class _Encounters:
    """`encounters` for the ensemble classes without tracers: the class keeps `_n_worlds`, its handle has `encounters`; a class of
    worlds of different sizes keeps `_cuts` (and `_tcuts` for its tracers) and gets per-world lists, as from `particles()`."""

    def _encounters(self, limit2, tracers, rows):
        limit2, tracers, rows = _checked_encounters(type(self).__name__, self._n_worlds, limit2, tracers, rows)
        out, *flat = self.h.encounters(limit2, tracers, rows)
        if not rows:
            return out, None, None, None
        if hasattr(self, "_cuts"):
            return (out, *([w.copy() for w in np.split(a, self._tcuts if tracers else self._cuts)] for a in flat))
        return (out, *(a.reshape(self._n_worlds, a.size // self._n_worlds) for a in flat))

    def encounters(self, limit2=None, rows=True):
        """-> (records, nn_index, nn_d2, close): ENCOUNTERS_DTYPE[B], and per body its nearest neighbour's world-local index (-1:
        none), its squared distance in the class's dtype (+inf: none) and the number of its pairs with d2 < limit2[k] — [B, n]
        arrays, or per-world lists where the worlds have sizes of their own; None each with rows=False.  limit2: None (the clamp
        of every world) or one number per world.  Bit for bit `encounters_of` of that world's rows.  The arguments are checked
        here, with ValueError, before the library is touched; the state is untouched."""
        return self._encounters(limit2, False, rows)


class _EncountersWithTracers(_Encounters):
    """`encounters` for the ensemble classes with tracers."""

    def encounters(self, limit2=None, tracers=False, rows=True):
        """-> (records, nn_index, nn_d2, close) as the classes without tracers give them; with tracers=True the targets are every
        world's tracers and the sources its bodies: per tracer the nearest body ([B, m] arrays or per-world lists; a world
        without tracers: rows == 0).  The arguments are checked here, with ValueError, before the library is touched; the state
        is untouched."""
        return self._encounters(limit2, tracers, rows)


WATCH_DTYPE = _capi.WATCH_DTYPE
WATCH_NEVER = _capi.WATCH_NEVER
WATCH_ROWS = _capi.WATCH_ROWS


def _checked_watch(who, b, dtype, delta, n_steps, limit2, height, stride, rows, resume, tracers, what="watch"):
    """The arguments of `watch` for b worlds -> (delta, n_steps, stride, limit2 float32[b] contiguous or None, height, tracers,
    resume, rows); ValueError naming `who` and the argument for anything else."""
    if isinstance(delta, (bool, np.bool_)) or not isinstance(delta, (int, float, np.integer, np.floating)):
        raise ValueError(f"{who}.{what}: delta must be a number, got {delta!r}")
    for name, v, least in (("n_steps", n_steps, 0), ("stride", stride, 1)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not least <= int(v) < 1 << 31:
            raise ValueError(f"{who}.{what}: {name} must be an integer {least} .. 2^31 - 1, got {v!r}")
    if isinstance(height, (bool, np.bool_)) or not isinstance(height, (int, np.integer)) or not 0 <= int(height) <= MAX_HEIGHT:
        raise ValueError(f"{who}.{what}: height must be an integer 0 .. 2^24, got {height!r}")
    for name, flag in (("rows", rows), ("resume", resume), ("tracers", tracers)):
        if not isinstance(flag, (bool, np.bool_)):
            raise ValueError(f"{who}.{what}: {name} must be True or False, got {flag!r}")
    if limit2 is not None:
        limit2 = np.asarray(limit2)
        if limit2.ndim != 1 or limit2.shape[0] != b:
            raise ValueError(f"{who}.{what}: limit2 must hold one squared distance per world ({b} worlds), got shape {limit2.shape}")
        if limit2.dtype.kind not in "fiu":
            raise ValueError(f"{who}.{what}: limit2 must be real numbers, got {limit2.dtype}")
        with np.errstate(over="ignore"):
            limit2 = np.ascontiguousarray(limit2, dtype=np.float32)
    return float(dtype(delta)), int(n_steps), int(stride), limit2, int(height), bool(tracers), bool(resume), bool(rows)


def _min_record(d2, sample):
    """The row with the smallest (d2, sample, row) among the rows with sample != WATCH_NEVER, or -1."""
    have = np.flatnonzero(sample != WATCH_NEVER)
    if not have.size:
        return -1
    order = np.lexsort((have, sample[have], d2[have].astype(np.float64)))   # (the last key sorts first)
    return int(have[order[0]])


def watch_merge(first, second, steps_before):
    """`watch(n1)` and the `watch(n2, resume=True)` that followed it, as one `watch(n1 + n2)`: first and second are what the two
    calls returned, (records, rows) with rows not None, and steps_before is n1 (a multiple of the stride) -> (records, rows), bit
    for bit what the one call gives.  The second call's sample numbers are shifted by steps_before; per target its closest
    approach replaces the first call's on a strict `<` only, first_close and first_out are the first call's unless it has none,
    close_samples add; the records are made again from the merged rows.  Plain NumPy: no GPU and no library call."""
    (rec1, rows1), (rec2, rows2) = first, second
    if rows1 is None or rows2 is None:
        raise ValueError("watch_merge: both calls must have returned their rows (rows=True): the records alone do not merge")
    if isinstance(steps_before, (bool, np.bool_)) or not isinstance(steps_before, (int, np.integer)) or not 0 <= int(steps_before) < 1 << 31:
        raise ValueError(f"watch_merge: steps_before must be an integer 0 .. 2^31 - 1, got {steps_before!r}")
    rec1, rec2 = np.asarray(rec1), np.asarray(rec2)
    if rec1.dtype != WATCH_DTYPE or rec2.dtype != WATCH_DTYPE or rec1.shape != rec2.shape or rec1.ndim != 1:
        raise ValueError("watch_merge: the records must be WATCH_DTYPE arrays of one length")
    for name in ("rows", "sources"):
        if not np.array_equal(rec1[name], rec2[name]):
            raise ValueError(f"watch_merge: the two calls differ in {name}: they are not calls on the same worlds")
    shift = np.uint32(int(steps_before))

    def later(s):
        return np.where(s == WATCH_NEVER, np.uint32(WATCH_NEVER), s + shift).astype(np.uint32)

    def world(a, b):
        take = (b["min_index"] >= 0) & ((a["min_index"] < 0) | (b["min_d2"] < a["min_d2"]))
        out = {"min_d2": np.where(take, b["min_d2"], a["min_d2"]), "min_index": np.where(take, b["min_index"], a["min_index"]),
               "min_sample": np.where(take, later(b["min_sample"]), a["min_sample"]),
               "close_samples": a["close_samples"] + b["close_samples"]}
        for name in ("first_close", "first_out"):
            out[name] = np.where(a[name] != WATCH_NEVER, a[name], later(b[name]))
        return {name: out[name].astype(a[name].dtype) for name in WATCH_ROWS}

    ragged = isinstance(rows1["min_d2"], list)
    n = rec1.shape[0]
    per_world = [world({k: rows1[k][i] for k in WATCH_ROWS}, {k: rows2[k][i] for k in WATCH_ROWS}) for i in range(n)]
    rec = rec1.copy()
    rec["samples"] = rec1["samples"] + rec2["samples"]
    for i, r in enumerate(per_world):
        at = _min_record(r["min_d2"], r["min_sample"])
        rec["min_row"][i] = at
        rec["min_source"][i] = r["min_index"][at] if at >= 0 else -1
        rec["min_sample"][i] = r["min_sample"][at] if at >= 0 else -1
        rec["min_d2"][i] = r["min_d2"][at] if at >= 0 else np.inf
        rec["close_rows"][i] = int((r["close_samples"] > 0).sum())
        rec["close_row_samples"][i] = int(r["close_samples"].astype(np.int64).sum())
        rec["out_rows"][i] = int((r["first_out"] != WATCH_NEVER).sum())
        rec["isolated_rows"][i] = int((r["min_index"] < 0).sum())
        for field, name in (("first_close_sample", "first_close"), ("first_out_sample", "first_out")):
            seen = r[name][r[name] != WATCH_NEVER]
            rec[field][i] = int(seen.min()) if seen.size else -1
    if ragged:
        return rec, {name: [r[name] for r in per_world] for name in WATCH_ROWS}
    return rec, {name: np.stack([r[name] for r in per_world]) for name in WATCH_ROWS}


class _Watch:
    """`watch` for the ensemble classes without tracers: the class keeps `_n_worlds` and `_dtype`, its handle has `watch`; a class
    of worlds of different sizes keeps `_cuts` (and `_tcuts` for its tracers) and gets per-world lists, as from `particles()`."""

    def _watch(self, delta, n_steps, limit2, height, stride, rows, resume, counter, tracers):
        delta, n_steps, stride, limit2, height, tracers, resume, rows = _checked_watch(
            type(self).__name__, self._n_worlds, self._dtype, delta, n_steps, limit2, height, stride, rows, resume, tracers)
        out, flat = self.h.watch(delta, n_steps, stride, limit2, height, tracers, resume, rows, counter)
        if not rows:
            return out, None
        if hasattr(self, "_cuts"):
            return out, {name: [w.copy() for w in np.split(a, self._tcuts if tracers else self._cuts)] for name, a in flat.items()}
        return out, {name: a.reshape(self._n_worlds, a.size // self._n_worlds) for name, a in flat.items()}

    def watch(self, delta, n_steps=1, limit2=None, height=0, stride=1, rows=True, resume=False, counter: Counting | None = None):
        """update(delta, n_steps) with every world sampled on the device before, between and after its steps (nbody_watch_*) ->
        (records, rows): WATCH_DTYPE[B] and a dict of six arrays per body — min_d2, min_index, min_sample: its closest approach
        to another body of its world over the samples, the source's world-local index and the sample it occurred at;
        first_close, close_samples: the first sample at which it had a pair with d2 < limit2[k] and how many samples had one;
        first_out: the first sample at which it was outside [0, height)^2 — [B, n] arrays, or per-world lists where the worlds
        have sizes of their own; None with rows=False.  Sample s is the state after s steps of this call, taken when s % stride
        == 0; resume=True leaves sample 0 out (`watch_merge` joins such a call to the one before it).  A sample number that did
        not occur is WATCH_NEVER in the rows and -1 in the records.  limit2: None (the clamp of every world) or one number per
        world.  The rows afterwards are bit for bit those after update(delta, n_steps=n_steps).  The arguments are checked here,
        with ValueError, before the library is touched."""
        return self._watch(delta, n_steps, limit2, height, stride, rows, resume, counter, False)


class _WatchWithTracers(_Watch):
    """`watch` for the ensemble classes with tracers."""

    def watch(self, delta, n_steps=1, limit2=None, height=0, stride=1, rows=True, resume=False, counter: Counting | None = None,
              tracers=False):
        """-> (records, rows) as the classes without tracers give them; with tracers=True the targets are every world's tracers
        and the sources its bodies: per tracer its closest approach to a body, its close samples and the sample at which it left
        the frame ([B, m] arrays or per-world lists; a world without tracers: rows == 0).  Bodies and tracers are stepped
        either way.  The arguments are checked here, with ValueError, before the library is touched."""
        return self._watch(delta, n_steps, limit2, height, stride, rows, resume, counter, tracers)


def _checked_watch_sweep(who, b, dtype, delta, clamp, steps, n_steps, stride, limit2, height, rows, resume, tracers):
    """The arguments of `watch_sweep` for b worlds -> (delta dtype[b], clamp float32[b] or None, steps int32[b] or None, n_steps,
    stride int32[b], limit2 float32[b] or None, height, tracers, resume, rows): the sweep's arguments as `sweep` checks them, the
    watch's as `watch` does, and stride a whole number >= 1 or one per world; ValueError naming `who` and the argument."""
    what = "watch_sweep"
    delta, clamp, steps, n_steps = _checked_sweep(who, b, dtype, delta, clamp, steps, n_steps, what)
    _, _, _, limit2, height, tracers, resume, rows = _checked_watch(who, b, dtype, 0.0, n_steps, limit2, height, 1, rows, resume, tracers, what)
    stride = np.asarray(stride)
    if stride.ndim == 0:
        stride = np.full(b, stride)
    if stride.ndim != 1 or stride.shape[0] != b:
        raise ValueError(f"{who}.{what}: stride must be one number or hold one per world ({b} worlds), got shape {stride.shape}")
    if stride.dtype.kind not in "iu":
        raise ValueError(f"{who}.{what}: stride must be integers, got {stride.dtype}")
    bad = np.flatnonzero((stride < 1) | (stride >= 1 << 31))
    if bad.size:
        k = int(bad[0])
        raise ValueError(f"{who}.{what}: stride[{k}] = {stride[k]} of world {k} must be 1 .. 2^31 - 1")
    return delta, clamp, steps, n_steps, np.ascontiguousarray(stride, dtype=np.int32), limit2, height, tracers, resume, rows


def watch_sweep_plan(steps, n_steps, stride=1, resume=False):
    """What `watch_sweep(..., steps=steps, n_steps=n_steps, stride=stride, resume=resume)` samples (nbody_wsweep_plan, pure host
    code, no GPU) -> (samples int64[B], launches): world k's number of samples — steps[k] // stride[k] + 1, one fewer with
    resume — and the number of s in 0 .. n_steps at which at least one world takes a sample, each of which costs one sampling
    launch.  steps: [B] integers; stride: one number or [B]."""
    steps = np.asarray(steps)
    if steps.ndim != 1 or steps.shape[0] < 1:
        raise ValueError(f"watch_sweep_plan: steps must hold one number per world, got shape {steps.shape}")
    b = steps.shape[0]
    _, _, steps, n_steps, stride, _, _, _, resume, _ = _checked_watch_sweep(
        "ensemble", b, np.float32, np.zeros(b, np.float32), None, steps, n_steps, stride, None, 0, True, resume, False)
    return _capi.wsweep_plan(b, steps, n_steps, stride, resume)


class _WatchSweep:
    """`watch_sweep` for the ensemble classes without tracers: what `_Watch` asks of the class, and a handle with `watch_sweep`."""

    def _watch_sweep(self, delta, clamp, steps, n_steps, stride, limit2, height, rows, resume, counter, tracers):
        delta, clamp, steps, n_steps, stride, limit2, height, tracers, resume, rows = _checked_watch_sweep(
            type(self).__name__, self._n_worlds, self._dtype, delta, clamp, steps, n_steps, stride, limit2, height, rows, resume, tracers)
        out, flat = self.h.watch_sweep(delta, clamp, steps, n_steps, stride, limit2, height, tracers, resume, rows, counter)
        if not rows:
            return out, None
        if hasattr(self, "_cuts"):
            return out, {name: [w.copy() for w in np.split(a, self._tcuts if tracers else self._cuts)] for name, a in flat.items()}
        return out, {name: a.reshape(self._n_worlds, a.size // self._n_worlds) for name, a in flat.items()}

    def watch_sweep(self, delta, clamp=None, steps=None, n_steps=None, stride=1, limit2=None, height=0, rows=True, resume=False,
                    counter: Counting | None = None):
        """sweep(delta, clamp, steps, n_steps=n_steps) with every world sampled on the device on its own schedule
        (nbody_wsweep_*) -> (records, rows) in the shapes `watch` returns.  World k takes sample s — the state after s steps of
        this call — iff s <= steps[k], s % stride[k] == 0 and not (s == 0 with resume=True); once it has taken its steps it
        stands still and is not sampled again, and its record's `samples` is its own steps[k] // stride[k] + 1 (one fewer with
        resume).  stride: one number or [B].  limit2: None (world k's own clamp[k]; without clamp the constructor's) or one
        number per world.  n_steps defaults as `sweep`'s does.  World k's record and rows are bit for bit those of this class
        holding world k alone with clamp[k], from watch(delta[k], steps[k], stride=stride[k], limit2 = limit2[k:k+1] or None);
        a world that takes no sample has samples == 0 and the empty rows (+inf, -1, WATCH_NEVER, WATCH_NEVER, 0, WATCH_NEVER).
        The rows afterwards are bit for bit those after sweep(delta, clamp, steps, n_steps=n_steps).  `watch_merge` joins a call
        and the resume=True call that continued it where every world either ran through the first call on a stride dividing
        its length or was finished within it; `watch_sweep_plan` says how many samples and sampling launches a schedule costs.
        The arguments are checked here, with ValueError, before the library is touched."""
        return self._watch_sweep(delta, clamp, steps, n_steps, stride, limit2, height, rows, resume, counter, False)


class _WatchSweepWithTracers(_WatchSweep):
    """`watch_sweep` for the ensemble classes with tracers."""

    def watch_sweep(self, delta, clamp=None, steps=None, n_steps=None, stride=1, limit2=None, height=0, rows=True, resume=False,
                    counter: Counting | None = None, tracers=False):
        """-> (records, rows) as the classes without tracers give them; with tracers=True the targets are every world's tracers
        and the sources its bodies, on the world's own schedule.  Bodies and tracers are stepped either way.  The arguments are
        checked here, with ValueError, before the library is touched."""
        return self._watch_sweep(delta, clamp, steps, n_steps, stride, limit2, height, rows, resume, counter, tracers)


class _Sweep:
    """`sweep` for every ensemble class: the class keeps `_n_worlds` and `_dtype`, its handle has `sweep`."""

    def sweep(self, delta, clamp=None, steps=None, counter: Counting | None = None, n_steps=None):
        """An update with a time step, a clamp and a number of steps per world (nbody_sweep_*): delta [B] (required), clamp [B]
        or None (the constructor's clamp in every world), steps [B] integers or None (every world takes n_steps).  World k takes
        the first steps[k] of the call's n_steps steps — n_steps defaults to max(steps), or 1 without steps — and then stands
        still bit for bit; its bits are those of this class holding world k alone with clamp[k], stepped by update(delta[k],
        n_steps=steps[k]).  The arguments are checked here, with ValueError, before the library is touched."""
        args = _checked_sweep(type(self).__name__, self._n_worlds, self._dtype, delta, clamp, steps, n_steps)
        self.h.sweep(*args, counter)


class _Resident:
    """`run` for the ensemble classes without tracers: the class keeps `_n_worlds` and `_dtype`, its handle has `resident`."""

    def run(self, delta, n_steps=None, clamp=None, steps=None, counter: Counting | None = None):
        """`sweep(delta, clamp, steps, n_steps=n_steps)` as a resident run (nbody_resident_*): every world is one block that
        keeps its positions and velocities in LDS and takes up to 1024 of its steps per launch, instead of one launch per step.
        delta is one time step for every world or one per world [B]; clamp, steps and n_steps are `sweep`'s.  The rows, the step
        count and the delta-stream sequence afterwards are bit for bit those after that `sweep`.  Worlds of at most 256 bodies
        only: the library refuses the call otherwise, and nothing moves.  The arguments are checked here, with ValueError, before
        the library is touched."""
        if delta is not None and np.ndim(delta) == 0:
            delta = np.full(self._n_worlds, delta)
        args = _checked_sweep(type(self).__name__, self._n_worlds, self._dtype, delta, clamp, steps, n_steps, "run")
        self.h.resident(*args, counter)


def _checked(position, velocity, weight, dtype=np.float32, who=None, other=None):
    """-> (B, n, position[B,n,2], velocity[B,n,2], weight[B,n] or None), contiguous; ValueError for anything else.  The
    messages name `who`, or the class of that dtype: Ensemble (float32) or Ensemble64 (float64); a wrong dtype adds `other`, or
    which of those two takes the other one."""
    position, velocity = np.asarray(position), np.asarray(velocity)
    dtype = np.dtype(dtype)
    name, sibling = ("Ensemble", "Ensemble64 takes float64") if dtype == np.float32 else ("Ensemble64", "Ensemble takes float32")
    who, other = who or name, other or sibling
    for name, a in (("position", position), ("velocity", velocity)):
        if a.dtype != dtype:
            raise ValueError(f"{who}: {name} must be {dtype} (got {a.dtype}); {other}")
    if position.ndim == 2:   # one world
        position = position[None]
        if velocity.ndim == 2:
            velocity = velocity[None]
        if weight is not None and np.ndim(weight) == 1:
            weight = np.asarray(weight)[None]
    if position.ndim != 3 or position.shape[2] != 2:
        raise ValueError(f"{who}: position must be [B, n, 2] (or [n, 2] for one world), got {position.shape}")
    if velocity.shape != position.shape:
        raise ValueError(f"{who}: velocity {velocity.shape} does not match position {position.shape}")
    b, n = position.shape[:2]
    if b < 1:
        raise ValueError(f"{who}: at least one world")
    if not 1 <= n <= MAX_BODIES:
        raise ValueError(f"{who}: 1 .. {MAX_BODIES} bodies per world, got {n} (above that a World per world is the tool)")
    if b * n > MAX_ROWS:
        raise ValueError(f"{who}: worlds * bodies = {b * n} exceeds 2^26")
    if weight is not None:
        weight = np.asarray(weight)
        if weight.shape != (b, n):
            raise ValueError(f"{who}: weight must be [B, n] = {(b, n)}, got {weight.shape}")
        if weight.dtype.kind not in "ui":
            raise ValueError(f"{who}: weight must be an integer array (u32 upstream), got {weight.dtype}")
        weight = np.ascontiguousarray(weight, dtype=np.uint32)
    return b, n, np.ascontiguousarray(position), np.ascontiguousarray(velocity), weight


class _EnsembleBase(_WatchSweep, _Watch, _Encounters, _Summary, _Sweep):
    """What Ensemble, Ensemble64 and the restricted ensembles share; each names its dtype and makes its own kind of handle."""
    _dtype = None

    @staticmethod
    def _new_handle(device):
        raise NotImplementedError

    def __init__(self, position, velocity, weight=None, *, device=0, clamp=0.001, arith="auto"):
        """position, velocity [B, n, 2] of the class's dtype (2-D: one world), weight [B, n] integers or None (all 1)."""
        if arith not in _ARITH:
            raise ValueError(f"arith must be one of {sorted(_ARITH)}")
        self.h = None
        args = _checked(position, velocity, weight, self._dtype)
        self.h = self._new_handle(device)
        self.h.set_params(clamp=float(clamp), arith=_ARITH[arith])
        self._upload(*args)

    def _upload(self, b, n, position, velocity, weight):
        self.h.upload(b, n, position, velocity, weight)
        self._n_worlds = b
        self._weight = np.ones((b, n), np.uint32) if weight is None else weight.copy()

    def upload(self, position, velocity, weight=None):
        """Replaces the ensemble by another one, of any shape."""
        self._upload(*_checked(position, velocity, weight, self._dtype))

    @property
    def shape(self):
        """(worlds, bodies per world)."""
        return self.h.shape

    def update(self, delta: float, counter: Counting | None = None, n_steps: int = 1):
        """n_steps direct steps of every world (World::update, main.rs:388-425, with the direct sum as its force phase); the
        call's seconds go to counter.sum_gravity."""
        self.h.update(delta, n_steps, counter)

    def particles(self):
        """-> (position[B,n,2], velocity[B,n,2], weight[B,n]); rows never move."""
        pos, vel = self.h.download()
        return pos, vel, self._weight.copy()

    def accel(self):
        """-> acc[B,n,2]: the accelerations at the current positions; the state is untouched."""
        return self.h.accel()

    def frames(self, height=100_000, render_px=100):
        """-> uint8 [B, render_px, render_px, 4]: the reference's draw() of every world's current rows, each world alone on its
        own tile, byte for byte `World.frame` of that world; the state is untouched."""
        return self.h.frames(height, render_px)

    def deltas(self, key=False):
        """-> (streams, step): one NBD1 delta stream (bytes) per world of the current positions, byte for byte what a `World` of
        that world alone hands out, and the steps taken so far.  The first call after an upload, and any call with key=True,
        gives key frames; `DeltasDecoder` follows the sequence.  The state is untouched."""
        return _streams(self.h, False, key)

    def close(self):
        if getattr(self, "h", None) is not None:
            self.h.close()
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Ensemble(_Resident, _EnsembleBase):
    """The ensemble in single precision: position, velocity [B, n, 2] float32."""
    _dtype = np.float32

    @staticmethod
    def _new_handle(device):
        return _capi.EnsembleHandle(device)


class Ensemble64(_Resident, _EnsembleBase):
    """The ensemble in double precision: position, velocity [B, n, 2] float64.  arith "auto" and "exact" are the exact chain;
    "fast" is opt-in and gated per world and per step on the device; clamp is a float, widened to double by the library."""
    _dtype = np.float64

    @staticmethod
    def _new_handle(device):
        return _capi.Ensemble64Handle(device)


def _checked_tracers(tracers, b, who="RestrictedEnsemble", dtype=np.float32):
    """tracers: None or (position[B,m,2], velocity[B,m,2]) of `dtype` ([m,2] for one world) -> (m, position, velocity), contiguous
    (m == 0: no tracers); ValueError for anything else."""
    if tracers is None:
        return 0, None, None
    if not isinstance(tracers, (tuple, list)) or len(tracers) != 2:
        raise ValueError(f"{who}: tracers must be a pair (position[B, m, 2], velocity[B, m, 2])")
    tp, tv = np.asarray(tracers[0]), np.asarray(tracers[1])
    dtype = np.dtype(dtype)
    other = "" if dtype == np.float32 else "; RestrictedEnsemble takes float32"
    for name, a in (("tracer position", tp), ("tracer velocity", tv)):
        if a.dtype != dtype:
            raise ValueError(f"{who}: {name} must be {dtype} (got {a.dtype}){other}")
    if tp.ndim == 2 and b == 1:
        tp = tp[None]
        if tv.ndim == 2:
            tv = tv[None]
    if tp.ndim != 3 or tp.shape[2] != 2:
        raise ValueError(f"{who}: tracer position must be [B, m, 2] (or [m, 2] for one world), got {tp.shape}")
    if tv.shape != tp.shape:
        raise ValueError(f"{who}: tracer velocity {tv.shape} does not match tracer position {tp.shape}")
    if tp.shape[0] != b:
        raise ValueError(f"{who}: tracers of {tp.shape[0]} worlds beside bodies of {b} worlds")
    m = tp.shape[1]
    if b * m > MAX_ROWS:
        raise ValueError(f"{who}: worlds * tracers = {b * m} exceeds 2^26")
    return m, np.ascontiguousarray(tp), np.ascontiguousarray(tv)


class _RestrictedBase(_WatchSweepWithTracers, _WatchWithTracers, _EncountersWithTracers, _SummaryWithTracers, _EnsembleBase):
    """What RestrictedEnsemble and RestrictedEnsemble64 share: the tracers beside the bodies.  Each names its dtype, makes its own
    kind of handle and says which class takes the other dtype."""
    _other = None

    def _check(self, position, velocity, weight, tracers):
        who = type(self).__name__
        args = _checked(position, velocity, weight, self._dtype, who=who, other=self._other)
        return args, _checked_tracers(tracers, args[0], who, self._dtype)

    def __init__(self, position, velocity, weight=None, tracers=None, *, device=0, clamp=0.001, arith="auto"):
        if arith not in _ARITH:
            raise ValueError(f"arith must be one of {sorted(_ARITH)}")
        self.h = None
        args, tr = self._check(position, velocity, weight, tracers)
        self.h = self._new_handle(device)
        self.h.set_params(clamp=float(clamp), arith=_ARITH[arith])
        self._upload(*args)
        self._upload_tracers(*tr)

    def _upload_tracers(self, m, tp, tv):
        self.h.upload_tracers(self.h.shape[0], m, tp, tv)

    def upload(self, position, velocity, weight=None, tracers=None):
        """Replaces the worlds by others, of any shape; the previous tracers go with them."""
        args, tr = self._check(position, velocity, weight, tracers)
        self._upload(*args)
        self._upload_tracers(*tr)

    def set_tracers(self, tracers):
        """Replaces the tracers: (position[B, m, 2], velocity[B, m, 2]); None, or m == 0, removes them."""
        self._upload_tracers(*_checked_tracers(tracers, self.h.shape[0], type(self).__name__, self._dtype))

    @property
    def shape(self):
        """(worlds, bodies per world, tracers per world)."""
        return (*self.h.shape, self.h.n_tracers)

    def tracers(self):
        """-> (position[B,m,2], velocity[B,m,2]) in upload order; rows never move."""
        return self.h.download_tracers()

    def tracers_accel(self):
        """-> acc[B,m,2]: the accelerations at the tracers' current positions; the state is untouched."""
        return self.h.tracers_accel()

    def frames(self, height=100_000, render_px=100, tracers=False):
        """-> uint8 [B, render_px, render_px, 4]: draw() of every world's bodies; tracers=True: followed by its tracers as rows
        of weight 1 (without tracers: the bodies' frames).  The state is untouched."""
        return self.h.frames(height, render_px, tracers)

    def deltas(self, tracers=False, key=False):
        """-> (streams, step): one NBD1 delta stream (bytes) per world, of the bodies' positions or, with tracers=True, of the
        tracers' (a sequence of its own; a world without tracers: a header of 0 rows), and the steps taken so far.  The first
        call after an upload of the rows it addresses, and any call with key=True, gives key frames.  The state is untouched."""
        return _streams(self.h, tracers, key)


class RestrictedEnsemble(_RestrictedBase):
    """B worlds of n bodies and m tracers each, float32: position, velocity [B, n, 2], weight [B, n] integers or None (all 1),
    tracers None or (position[B, m, 2], velocity[B, m, 2]).  Every update steps the bodies as `Ensemble` does, bit for bit, and
    the tracers in the field of their own world's bodies at the pre-step positions."""
    _dtype = np.float32

    @staticmethod
    def _new_handle(device):
        return _capi.RestrictedHandle(device)


class RestrictedEnsemble64(_RestrictedBase):
    """The restricted ensemble in double precision: the same constructor and methods, float64 arrays only.  Every update steps
    the bodies as `Ensemble64` does, bit for bit, and the tracers in double: arith "auto" and "exact" are the exact chain, "fast"
    is opt-in and gated per world and per step on the device, with a per-tracer exception for a tracer outside FAST's domain;
    clamp is a float, widened to double by the library."""
    _dtype = np.float64
    _other = "RestrictedEnsemble takes float32"

    @staticmethod
    def _new_handle(device):
        return _capi.Restricted64Handle(device)


def _checked_ragged(positions, velocities, weights, dtype=np.float32, who=None, other=None):
    """-> (sizes int64[B], position[rows,2], velocity[rows,2], weight uint32[rows] or None), the worlds' rows one after another;
    ValueError for anything else.  Nothing is copied before every world has passed.  The messages name `who`, or the class of
    that dtype: RaggedEnsemble (float32) or RaggedEnsemble64 (float64); a wrong dtype adds `other`, or which of those two takes
    the other one."""
    dtype = np.dtype(dtype)
    name, sibling = (("RaggedEnsemble", "RaggedEnsemble64 takes float64") if dtype == np.float32
                     else ("RaggedEnsemble64", "RaggedEnsemble takes float32"))
    who, other = who or name, other or sibling
    for name, seq in (("positions", positions), ("velocities", velocities)) + ((("weights", weights),) if weights is not None else ()):
        if not hasattr(seq, "__len__"):
            raise ValueError(f"{who}: {name} must be a sequence of per-world arrays")
    b = len(positions)
    if b < 1:
        raise ValueError(f"{who}: at least one world")
    if len(velocities) != b or (weights is not None and len(weights) != b):
        raise ValueError(f"{who}: positions, velocities and weights must be lists of equal length ({b} worlds)")
    sizes, rows = [], 0
    for k in range(b):
        p, v = np.asarray(positions[k]), np.asarray(velocities[k])
        for name, a in (("position", p), ("velocity", v)):
            if a.dtype != dtype:
                raise ValueError(f"{who}: world {k}: {name} must be {dtype} (got {a.dtype}); {other}")
        if p.ndim != 2 or p.shape[1] != 2:
            raise ValueError(f"{who}: world {k}: position must be [n, 2], got {p.shape}")
        if v.shape != p.shape:
            raise ValueError(f"{who}: world {k}: velocity {v.shape} does not match position {p.shape}")
        n = p.shape[0]
        if not 1 <= n <= MAX_BODIES:
            raise ValueError(f"{who}: world {k}: 1 .. {MAX_BODIES} bodies per world, got {n} (above that a World per world is the tool)")
        if weights is not None:
            w = np.asarray(weights[k])
            if w.shape != (n,):
                raise ValueError(f"{who}: world {k}: weight must be [n] = {(n,)}, got {w.shape}")
            if w.dtype.kind not in "ui":
                raise ValueError(f"{who}: world {k}: weight must be an integer array (u32 upstream), got {w.dtype}")
        sizes.append(n)
        rows += n
        if rows > MAX_ROWS:
            raise ValueError(f"{who}: the sizes add up to more than 2^26 rows")
    position = np.ascontiguousarray(np.concatenate([np.asarray(p) for p in positions]))
    velocity = np.ascontiguousarray(np.concatenate([np.asarray(v) for v in velocities]))
    weight = None if weights is None else np.ascontiguousarray(np.concatenate([np.asarray(w) for w in weights]), dtype=np.uint32)
    return np.asarray(sizes, np.int64), position, velocity, weight


class _RaggedBase(_WatchSweep, _Watch, _Encounters, _Summary, _Sweep):
    """What RaggedEnsemble and RaggedEnsemble64 share; each names its dtype, makes its own kind of handle and has its own
    constructor."""
    _dtype = None

    @staticmethod
    def _new_handle(device):
        raise NotImplementedError

    def _create(self, positions, velocities, weights, device, clamp, arith):
        if arith not in _ARITH:
            raise ValueError(f"arith must be one of {sorted(_ARITH)}")
        self.h = None
        args = _checked_ragged(positions, velocities, weights, self._dtype)
        self.h = self._new_handle(device)
        self.h.set_params(clamp=float(clamp), arith=_ARITH[arith])
        self._upload(*args)

    def _upload(self, sizes, position, velocity, weight):
        self.h.upload(sizes, position, velocity, weight)
        self._n_worlds = int(sizes.shape[0])
        self._sizes = sizes
        self._cuts = np.cumsum(sizes)[:-1]
        self._weight = np.ones(int(sizes.sum()), np.uint32) if weight is None else weight.copy()

    def upload(self, positions, velocities, weights=None):
        """Replaces the worlds by others, of any sizes."""
        self._upload(*_checked_ragged(positions, velocities, weights, self._dtype))

    def _per_world(self, a):
        return [w.copy() for w in np.split(a, self._cuts)]

    @property
    def sizes(self):
        """The bodies of every world, in world order."""
        return [int(n) for n in self._sizes]

    def update(self, delta: float, counter: Counting | None = None, n_steps: int = 1):
        """n_steps direct steps of every world; the call's seconds go to counter.sum_gravity."""
        self.h.update(delta, n_steps, counter)

    def particles(self):
        """-> (positions, velocities, weights): lists of per-world arrays [n_k, 2], [n_k, 2], [n_k]; rows never move."""
        pos, vel = self.h.download()
        return self._per_world(pos), self._per_world(vel), self._per_world(self._weight)

    def accel(self):
        """-> a list of acc[n_k, 2]: the accelerations at the current positions; the state is untouched."""
        return self._per_world(self.h.accel())

    def frames(self, height=100_000, render_px=100):
        """-> uint8 [B, render_px, render_px, 4]: the reference's draw() of every world's current rows, each world alone on its
        own tile, whatever its size; the state is untouched."""
        return self.h.frames(height, render_px)

    def deltas(self, key=False):
        """-> (streams, step): one NBD1 delta stream (bytes) per world of the current positions, byte for byte what a `World` of
        that world alone hands out, and the steps taken so far.  The first call after an upload, and any call with key=True,
        gives key frames; `DeltasDecoder` follows the sequence.  The state is untouched."""
        return _streams(self.h, False, key)

    def close(self):
        if getattr(self, "h", None) is not None:
            self.h.close()
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class RaggedEnsemble(_Resident, _RaggedBase):
    """Worlds of different sizes, stepped together: positions, velocities are sequences of [n_k, 2] float32 arrays, weights a
    sequence of [n_k] integer arrays or None (all 1).  1 .. 4096 bodies per world, at most 2^26 bodies in all."""
    _dtype = np.float32

    @staticmethod
    def _new_handle(device):
        return _capi.RaggedHandle(device)

    def __init__(self, positions, velocities, weights=None, *, device=0, clamp=0.001, arith="auto"):
        self._create(positions, velocities, weights, device, clamp, arith)


class RaggedEnsemble64(_Resident, _RaggedBase):
    """The ragged ensemble in double precision: positions, velocities are sequences of [n_k, 2] float64 arrays.  arith "exact"
    and "auto" are the exact chain; "fast" is opt-in and gated per world and per step on the device; clamp is a float, widened
    to double by the library."""
    _dtype = np.float64

    @staticmethod
    def _new_handle(device):
        return _capi.Ragged64Handle(device)

    def __init__(self, positions, velocities, weights=None, arith="exact", clamp=0.001, device=0):
        self._create(positions, velocities, weights, device, clamp, arith)


def _checked_rr_tracers(tracers, sizes, who="RaggedRestrictedEnsemble", dtype=np.float32, other=None):
    """tracers: None, or one entry per world, each None or a pair (position[m_k, 2], velocity[m_k, 2]) of `dtype` ->
    (counts int64[B], position[rows, 2], velocity[rows, 2]), the worlds' tracer rows one after another (both None where no
    world has a tracer); ValueError for anything else.  Nothing is copied before every world has passed.  A wrong dtype adds
    `other` to the message where one is given: which class takes the other one."""
    dtype = np.dtype(dtype)
    b = len(sizes)
    counts = np.zeros(b, np.int64)
    if tracers is None:
        return counts, None, None
    if not isinstance(tracers, (tuple, list)) or len(tracers) != b:
        raise ValueError(f"{who}: tracers must be None or a list with one entry per world ({b} worlds): None or a pair "
                         "(position[m, 2], velocity[m, 2])")
    tps, tvs, rows = [], [], 0
    for k, entry in enumerate(tracers):
        if entry is None:
            continue
        if not isinstance(entry, (tuple, list)) or len(entry) != 2:
            raise ValueError(f"{who}: world {k}: tracers must be None or a pair (position[m, 2], velocity[m, 2])")
        tp, tv = np.asarray(entry[0]), np.asarray(entry[1])
        for name, a in (("tracer position", tp), ("tracer velocity", tv)):
            if a.dtype != dtype:
                raise ValueError(f"{who}: world {k}: {name} must be {dtype} (got {a.dtype})" + (f"; {other}" if other else ""))
        if tp.ndim != 2 or tp.shape[1] != 2:
            raise ValueError(f"{who}: world {k}: tracer position must be [m, 2], got {tp.shape}")
        if tv.shape != tp.shape:
            raise ValueError(f"{who}: world {k}: tracer velocity {tv.shape} does not match tracer position {tp.shape}")
        counts[k] = tp.shape[0]
        rows += tp.shape[0]
        if rows > MAX_ROWS:
            raise ValueError(f"{who}: the tracers add up to more than 2^26 rows")
        if tp.shape[0]:
            tps.append(tp), tvs.append(tv)
    if not rows:
        return counts, None, None
    return counts, np.ascontiguousarray(np.concatenate(tps)), np.ascontiguousarray(np.concatenate(tvs))


class RaggedRestrictedEnsemble(_WatchSweepWithTracers, _WatchWithTracers, _EncountersWithTracers, _SummaryWithTracers, _RaggedBase):
    """Worlds of different sizes, each with tracers of its own, stepped together (nbody_rr_*), float32: positions, velocities
    are sequences of [n_k, 2] arrays, weights a sequence of [n_k] integer arrays or None (all 1), tracers None or a list with one
    entry per world, each None or a pair (position[m_k, 2], velocity[m_k, 2]).  1 .. 4096 bodies per world, at most 2^26 bodies
    and at most 2^26 tracers in all.  The bodies are bit-identical to a `RaggedEnsemble` of the same worlds; a tracer is EXACT
    bit-identical to the oracle's direct_accel at it + Euler, FAST bit-identical to a `RestrictedEnsemble` holding its world
    alone, AUTO per world and per step on the device with the per-tracer exception of `RestrictedEnsemble`."""
    _dtype = np.float32
    _who = "RaggedRestrictedEnsemble"
    _other = "it takes float32 only"  # what a wrong dtype of the bodies adds to the message
    _tracer_other = None              # and of the tracers

    @staticmethod
    def _new_handle(device):
        return _capi.RRHandle(device)

    def _check(self, positions, velocities, weights, tracers):
        args = _checked_ragged(positions, velocities, weights, self._dtype, who=self._who, other=self._other)
        return args, _checked_rr_tracers(tracers, args[0], self._who, self._dtype, self._tracer_other)

    def __init__(self, positions, velocities, weights=None, tracers=None, *, device=0, clamp=0.001, arith="auto"):
        if arith not in _ARITH:
            raise ValueError(f"{self._who}: arith must be one of {sorted(_ARITH)}")
        self.h = None
        args, tr = self._check(positions, velocities, weights, tracers)
        self.h = self._new_handle(device)
        self.h.set_params(clamp=float(clamp), arith=_ARITH[arith])
        self._upload(*args)
        self._upload_tracers(*tr)

    def _upload_tracers(self, counts, tp, tv):
        self.h.upload_tracers(counts, tp, tv)
        self._counts = counts
        self._tcuts = np.cumsum(counts)[:-1]

    def upload(self, positions, velocities, weights=None, tracers=None):
        """Replaces the worlds by others, of any sizes; the previous tracers go with them."""
        args, tr = self._check(positions, velocities, weights, tracers)
        self._upload(*args)
        self._upload_tracers(*tr)

    def set_tracers(self, tracers):
        """Replaces the tracers: a list with one entry per world, each None or (position[m_k, 2], velocity[m_k, 2]); None, or no
        tracer in any world, removes them."""
        self._upload_tracers(*_checked_rr_tracers(tracers, self._sizes, self._who, self._dtype, self._tracer_other))

    @property
    def sizes(self):
        """(the bodies of every world, the tracers of every world), in world order."""
        return [int(n) for n in self._sizes], [int(m) for m in self._counts]

    def _per_world_tracers(self, a):
        return [t.copy() for t in np.split(a, self._tcuts)]

    def tracers(self):
        """-> a list of pairs (position[m_k, 2], velocity[m_k, 2]) in upload order, empty arrays where m_k == 0; rows never move."""
        pos, vel = self.h.download_tracers()
        return list(zip(self._per_world_tracers(pos), self._per_world_tracers(vel)))

    def tracers_accel(self):
        """-> a list of acc[m_k, 2]: the accelerations at the tracers' current positions; the state is untouched."""
        return self._per_world_tracers(self.h.tracers_accel())

    def frames(self, height=100_000, render_px=100, tracers=False):
        """-> uint8 [B, render_px, render_px, 4]: draw() of every world's bodies; tracers=True: followed by its own tracers as
        rows of weight 1 (a world without tracers: its bodies).  The state is untouched."""
        return self.h.frames(height, render_px, tracers)

    def deltas(self, tracers=False, key=False):
        """-> (streams, step): one NBD1 delta stream (bytes) per world, of the bodies' positions or, with tracers=True, of the
        tracers' (a sequence of its own; a world without tracers: a header of 0 rows), and the steps taken so far.  The first
        call after an upload of the rows it addresses, and any call with key=True, gives key frames.  The state is untouched."""
        return _streams(self.h, tracers, key)


class RaggedRestrictedEnsemble64(RaggedRestrictedEnsemble):
    """The ragged restricted ensemble in double precision (nbody_rr64_*): the same constructor and methods, float64 arrays
    only.  The bodies are bit-identical to a `RaggedEnsemble64` of the same worlds; a tracer is under arith "exact" and "auto"
    (the exact chain, as for every float64 class) bit-identical to the oracle's float64 direct_accel at it + Euler, and under
    "fast" (opt-in, gated per world and per step on the device, with the per-tracer exception) bit-identical to a
    `RestrictedEnsemble64` holding its world alone.  clamp is a float, widened to double by the library."""
    _dtype = np.float64
    _who = "RaggedRestrictedEnsemble64"
    _other = _tracer_other = "RaggedRestrictedEnsemble takes float32"

    @staticmethod
    def _new_handle(device):
        return _capi.RR64Handle(device)


class DeltasDecoder:
    """The receiving side of `deltas()` (host only): one `DeltaDecoder` per world.  `apply(streams)` takes the list one call
    returned; a list of the wrong length is refused, and where a decoder's header checks refuse one stream none of the list is
    applied."""

    def __init__(self, n_worlds):
        n_worlds = int(n_worlds)
        if n_worlds < 1:
            raise ValueError(f"DeltasDecoder: at least one world, got {n_worlds}")
        self._decoders = [_capi.DeltaDecoder() for _ in range(n_worlds)]
        self.step = 0

    def __len__(self):
        return len(self._decoders)

    def apply(self, streams):
        if not isinstance(streams, (list, tuple)) or len(streams) != len(self._decoders):
            raise ValueError(f"DeltasDecoder: {len(self._decoders)} streams expected, one per world")
        for k, (d, s) in enumerate(zip(self._decoders, streams)):
            why = _refused(d, bytes(s))
            if why:
                raise _capi.NBodyError(_capi.ERR_INVALID, f"DeltasDecoder: world {k}: {why} (nothing applied)")
        for d, s in zip(self._decoders, streams):
            d.apply(s)
        if streams:
            self.step = self._decoders[0].step

    def positions(self):
        """-> a list of arrays [n_k, 2], one per world: the positions of the last applied streams."""
        return [d.positions() for d in self._decoders]

    def close(self):
        for d in self._decoders:
            d.close()


def _refused(decoder, stream):
    """What the header checks of nbody_delta_decoder_apply (csrc/delta_decoder.hpp) would say of `stream` in the state `decoder`
    is in, or None: restated here so that a list of streams can be checked whole before any of it is applied."""
    if len(stream) < 32 or stream[:4] != b"NBD1":
        return "not an NBD1 stream"
    bits, key = stream[4], stream[5]
    if bits not in (32, 64) or key > 1 or stream[6:8] != b"\0\0":
        return "bad header"
    n, total = int.from_bytes(stream[8:16], "little"), int.from_bytes(stream[24:32], "little")
    if n > 0x7fffffff:
        return "body count out of range"
    nblk = (n + 63) // 64
    wb = (2 * nblk + 7) // 8 * 8
    if total > 2 * nblk * bits or len(stream) != 32 + wb + 8 * total:
        return "the size does not match the header"
    if not key and (decoder.n != n or (decoder.dtype == np.float64) != (bits == 64)):
        return "a delta stream out of sequence"
    widths = np.frombuffer(stream, np.uint8, wb, 32)
    w = widths[:2 * nblk] & 127
    if (w > bits).any() or widths[2 * nblk:].any() or int(w.sum(dtype=np.int64)) != total:
        return "the width bytes do not match the payload"
    return None


def contact_sheet(frames, cols=None):
    """Tiles frames [W, px, px, 4] (what `frames()` returns) row-major into one image [ceil(W / cols) * px, cols * px, 4]: world k
    at tile (k // cols, k % cols).  cols defaults to ceil(sqrt(W)); tiles past the last world stay zero.  Pure numpy."""
    frames = np.asarray(frames)
    if frames.ndim != 4 or frames.shape[0] < 1 or frames.shape[1] != frames.shape[2]:
        raise ValueError(f"contact_sheet: frames must be [W, px, px, channels] with W >= 1, got {frames.shape}")
    w, px, _, ch = frames.shape
    if cols is None:
        cols = int(np.sqrt(w))
        cols += cols * cols < w      # ceil(sqrt(W)), in integers
    cols = int(cols)
    if cols < 1:
        raise ValueError(f"contact_sheet: cols must be >= 1, got {cols}")
    rows = -(-w // cols)
    sheet = np.zeros((rows * cols, px, px, ch), frames.dtype)
    sheet[:w] = frames
    return np.ascontiguousarray(sheet.reshape(rows, cols, px, px, ch).transpose(0, 2, 1, 3, 4).reshape(rows * px, cols * px, ch))


def rr_plan(sizes, tracer_counts, dtype=np.float32):
    """The launches the TRACERS of a RaggedRestrictedEnsemble (dtype float64: a RaggedRestrictedEnsemble64) of these sizes and
    tracer counts take per step (nbody_rr_plan / nbody_rr64_plan; host code, no GPU needed; the bodies' launches are
    `ragged_plan(sizes, dtype)`) -> dict: launch_of_world, first_block_of_world (a world's blocks are contiguous in its launch;
    both -1 for a world without tracers), lds_bytes and blocks per launch."""
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"rr_plan: dtype must be float32 or float64, got {dtype}")
    sizes, counts = [int(n) for n in sizes], [int(m) for m in tracer_counts]
    if not sizes or min(sizes) < 1 or max(sizes) > MAX_BODIES or sum(sizes) > MAX_ROWS:
        raise ValueError(f"rr_plan: at least one world, 1 .. {MAX_BODIES} bodies per world, at most 2^26 in all")
    if len(counts) != len(sizes) or min(counts) < 0 or sum(counts) > MAX_ROWS:
        raise ValueError("rr_plan: one tracer count >= 0 per world, at most 2^26 tracers in all")
    launch, first, lds, blocks = _capi.rr_plan(sizes, counts, f64=dtype == np.float64)
    return dict(launch_of_world=launch, first_block_of_world=first, lds_bytes=lds, blocks=blocks)


RESIDENT_MAX_BODIES = _capi.RESIDENT_MAX_BODIES                # per world of a resident run: one block
RESIDENT_STEPS_PER_LAUNCH = _capi.RESIDENT_STEPS_PER_LAUNCH    # of a resident run


def resident_plan(sizes, steps=None, n_steps=1, dtype=np.float32):
    """What `run(..., steps=steps, n_steps=n_steps)` on worlds of these sizes enqueues (nbody_resident_plan; host code, no GPU
    needed) -> dict: n_launches — ceil(max(steps) / 1024), 0 where no world takes a step — and lds_bytes, the dynamic LDS of a
    launch, which is that of the largest world.  steps is one count per world or None (every world takes n_steps)."""
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"resident_plan: dtype must be float32 or float64, got {dtype}")
    sizes = np.ascontiguousarray([int(n) for n in sizes], dtype=np.int64)
    if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or not -(1 << 31) <= int(n_steps) < 1 << 31:
        raise ValueError(f"resident_plan: n_steps must be an integer, got {n_steps!r}")
    if steps is not None:
        steps = np.asarray(steps)
        if steps.shape != sizes.shape or steps.dtype.kind not in "iu" or (steps.size and (steps.min() < -(1 << 31) or steps.max() >= 1 << 31)):
            raise ValueError(f"resident_plan: steps must hold one integer per world, got shape {steps.shape} of {steps.dtype}")
        steps = np.ascontiguousarray(steps, dtype=np.int32)
    launches, lds = _capi.resident_plan(sizes, steps, int(n_steps), dtype == np.float64)
    return dict(n_launches=launches, lds_bytes=lds)


def ragged_plan(sizes, dtype=np.float32):
    """The launches a RaggedEnsemble (dtype float64: a RaggedEnsemble64) of these sizes takes per step (nbody_ragged_plan /
    nbody_ragged64_plan; host code, no GPU needed) -> dict: launch_of_world, first_block_of_world (a world's blocks are
    contiguous in its launch), lds_bytes and blocks per launch."""
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"ragged_plan: dtype must be float32 or float64, got {dtype}")
    sizes = [int(n) for n in sizes]
    if not sizes or min(sizes) < 1 or max(sizes) > MAX_BODIES or sum(sizes) > MAX_ROWS:
        raise ValueError(f"ragged_plan: at least one world, 1 .. {MAX_BODIES} bodies per world, at most 2^26 in all")
    launch, first, lds, blocks = _capi.ragged_plan(sizes, f64=dtype == np.float64)
    return dict(launch_of_world=launch, first_block_of_world=first, lds_bytes=lds, blocks=blocks)
