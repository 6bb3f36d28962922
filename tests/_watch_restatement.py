"""The watch's contract (include/nbody_ensemble.h, "a watched run of an ensemble") restated in NumPy, independently of the
library: a world is a list of frames, one per taken sample — (sample number, targets[n, 2], sources[n_s, 2] or None: the targets
are the world's bodies) — and `world` folds them into the six per-target arrays and the record.  Per sample the nearest live
source comes from tests/_encounters_restatement.py: the class's dtype, unfused operations, `is normal` spelled out, ties by
explicit comparisons.  Two rivals for the host tests: `latest=True` lets a later sample stand on a tie in time, `highest=True`
keeps the highest source index of a tie.  `fold` is the part after the pairs: it takes every sample's (nn_index, nn_d2) and the
targets' positions, which is what the device test's loop over encounters() and particles() sees.  `merge` restates
nb.watch_merge, one target at a time.

Also here, because the host and the device tests share them: which samples a call takes (`taken`), straight-line frames
(`ballistic`), and the hand-computed worlds (`HAND`, `hand_world`, `static_lattice`)."""
import numpy as np

import _encounters_restatement as R
import _encounters_scene as S

NEVER = 0xffffffff
ROWS = ("min_d2", "min_index", "min_sample", "first_close", "close_samples", "first_out")
DTYPE = np.dtype([(name, np.int64) for name in ("rows", "sources", "samples", "min_row", "min_source", "min_sample")] +
                 [("min_d2", np.float64)] +
                 [(name, np.int64) for name in ("close_rows", "close_row_samples", "first_close_sample", "out_rows", "first_out_sample",
                                                "isolated_rows")])


def taken(n_steps, stride=1, resume=False):
    """The sample numbers a call takes."""
    return [s for s in range(n_steps + 1) if s % stride == 0 and not (s == 0 and resume)]


def empty_rows(n, dtype):
    return {"min_d2": np.full(n, np.inf, dtype), "min_index": np.full(n, -1, np.int32), "min_sample": np.full(n, NEVER, np.uint32),
            "first_close": np.full(n, NEVER, np.uint32), "close_samples": np.zeros(n, np.uint32), "first_out": np.full(n, NEVER, np.uint32)}


def record(rows, n_sources, samples):
    r = np.zeros(1, DTYPE)[0]
    n = rows["min_index"].shape[0]
    r["rows"], r["sources"], r["samples"] = n, n_sources, samples
    r["min_row"] = r["min_source"] = r["min_sample"] = r["first_close_sample"] = r["first_out_sample"] = -1
    r["min_d2"] = np.inf
    best = None
    for i in range(n):                                    # (d2, sample, row): rows ascend, so only a strictly smaller key replaces
        if rows["min_index"][i] < 0:
            r["isolated_rows"] += 1
            continue
        key = (float(rows["min_d2"][i]), int(rows["min_sample"][i]))
        if best is None or key < best:
            best = key
            r["min_row"], r["min_source"], r["min_sample"], r["min_d2"] = i, rows["min_index"][i], key[1], key[0]
    r["close_rows"] = int((rows["close_samples"] > 0).sum())
    r["close_row_samples"] = int(rows["close_samples"].astype(np.int64).sum())
    r["out_rows"] = int((rows["first_out"] != NEVER).sum())
    for field, name in (("first_close_sample", "first_close"), ("first_out_sample", "first_out")):
        seen = [int(v) for v in rows[name] if v != NEVER]
        if seen:
            r[field] = min(seen)
    return r


def world(frames, limit2, height, n_targets, n_sources, dtype, latest=False, highest=False):
    """-> (record, rows dict) of one world over its taken samples.  limit2: a float32, widened to the dtype as the handle widens
    it.  n_targets, n_sources, dtype: the world's, for a call that took no sample."""
    T = np.dtype(dtype).type
    seen = []
    for s, targets, sources in frames:
        own = sources is None
        idx, best, _, _ = R.rows(targets, targets if own else sources, own, T(np.float32(limit2)), highest=highest)
        seen.append((s, idx, best, targets))
    return fold(seen, limit2, height, n_targets, n_sources, dtype, latest=latest)


def fold(seen, limit2, height, n_targets, n_sources, dtype, latest=False):
    """-> (record, rows dict) from the taken samples' own answers: seen is a list of (sample number, nn_index, nn_d2, the
    targets' positions), what an encounters report and a download at that point give."""
    T = np.dtype(dtype).type
    rows = empty_rows(n_targets, T)
    limit, h = T(np.float32(limit2)), T(height)
    for s, idx, best, targets in seen:
        assert best.dtype == np.dtype(T) and targets.dtype == np.dtype(T)
        has = idx >= 0
        with np.errstate(invalid="ignore"):
            close = has & (best < limit)
            x, y = targets[:, 0], targets[:, 1]
            out = ~((y < h) & (x < h) & (y >= T(0)) & (x >= T(0)))                       # within_bounds; NaN fails
            better = (best <= rows["min_d2"]) if latest else (best < rows["min_d2"])
        take = has & ((rows["min_index"] < 0) | better)
        rows["min_d2"] = np.where(take, best, rows["min_d2"])
        rows["min_index"] = np.where(take, idx, rows["min_index"]).astype(np.int32)
        rows["min_sample"] = np.where(take, np.uint32(s), rows["min_sample"]).astype(np.uint32)
        rows["first_close"] = np.where(close & (rows["first_close"] == NEVER), np.uint32(s), rows["first_close"]).astype(np.uint32)
        rows["close_samples"] = (rows["close_samples"] + close).astype(np.uint32)
        rows["first_out"] = np.where(out & (rows["first_out"] == NEVER), np.uint32(s), rows["first_out"]).astype(np.uint32)
    assert rows["min_d2"].dtype == np.dtype(T)
    return record(rows, n_sources, len(seen)), rows


def merge(first, second, steps_before):
    """(record, rows) of one world from watch(n1) and from the watch(n2, resume) after it -> those of watch(n1 + n2)."""
    (rec1, a), (rec2, b) = first, second
    n = a["min_index"].shape[0]
    rows = {name: a[name].copy() for name in ROWS}

    def later(v):
        return NEVER if v == NEVER else int(v) + steps_before

    for i in range(n):
        if b["min_index"][i] >= 0 and (a["min_index"][i] < 0 or b["min_d2"][i] < a["min_d2"][i]):
            rows["min_d2"][i], rows["min_index"][i], rows["min_sample"][i] = b["min_d2"][i], b["min_index"][i], later(b["min_sample"][i])
        for name in ("first_close", "first_out"):
            if a[name][i] == NEVER:
                rows[name][i] = later(b[name][i])
        rows["close_samples"][i] = int(a["close_samples"][i]) + int(b["close_samples"][i])
    return record(rows, int(rec1["sources"]), int(rec1["samples"]) + int(rec2["samples"])), rows


def same(a, b):
    return R.same(a, b)


def same_world(got, want):
    """Bit for bit: (record, rows dict) against (record, rows dict)."""
    return same(got[0], want[0]) and all(same(got[1][name], want[1][name]) for name in ROWS)


def diff(got, want):
    """The names of what differs, for a failure message."""
    return [f for f in DTYPE.names if not same(got[0][f], want[0][f])] + [name for name in ROWS if not same(got[1][name], want[1][name])]


# ---- straight lines: what weight-0 bodies, and tracers over them, do under EXACT
def ballistic(pos, vel, delta, n_steps):
    """-> [n_steps + 1] position arrays: x += v * delta per step in the arrays' dtype (exact for the dyadic numbers used here)."""
    T = pos.dtype.type
    out, p = [pos.copy()], pos.copy()
    for _ in range(n_steps):
        p = p + vel * T(delta)
        out.append(p.copy())
    return out


def frames_of(samples, targets, sources=None):
    """targets, sources: per-sample position lists (sources None: the targets are the bodies) -> the frames `world` takes."""
    return [(s, targets[s], None if sources is None else sources[s]) for s in samples]


# The hand-computed world: delta = 0.5, five steps, limit2 = 1.5, height = 64.  Bodies (weight 0 on the device):
#   0, 1   body 0 passes body 1: d2 = (3 - s)^2 + 1 = 10 5 2 1 2 5: the minimum 1 at the middle sample 3, close at s = 3 alone
#   2, 3   body 2 passes body 3: d2 = (2.5 - s)^2 + 1 = 7.25 3.25 1.25 1.25 3.25 7.25: a tie in time, the earlier sample 2
#          stands; close at exactly the samples 2 and 3
#   4      leaves the frame: x = 2 1 0 -1 -2 -3, out from sample 3 on (x = 0 is inside)
#   5      begins outside and comes in: x = -2 -1 0 1 2 3, out at the samples 0 and 1 and inside afterwards: first_out stays 0
#          (bodies 4 and 5 are nearest to each other: d2 = (2s - 4)^2 + 25, 25 at sample 2)
# Tracers (the restricted classes), against those bodies:
#   0      passes body 1 at d2 = (3 - s)^2 + 1 while body 0 rides along at d2 = 4: minimum 1 at sample 3, source 1
#   1      leaves the frame at sample 3; its nearest body is body 4 straight above it, d2 = 100 at every sample: sample 0 stands
#   2      passes body 3 at d2 = (2.5 - s)^2 + 1 while body 2 rides along at d2 = 4: 1.25 at the samples 2 and 3, sample 2 stands
HAND = dict(delta=0.5, n_steps=5, limit2=1.5, height=64,
            pos=[[10, 10], [13, 11], [10, 30], [12.5, 31], [2, 50], [-2, 55]],
            vel=[[2, 0], [0, 0], [2, 0], [0, 0], [-2, 0], [2, 0]],
            tpos=[[10, 12], [2, 40], [10, 32]],
            tvel=[[2, 0], [-2, 0], [2, 0]],
            bodies=dict(min_d2=[1, 1, 1.25, 1.25, 25, 25], min_index=[1, 0, 3, 2, 5, 4], min_sample=[3, 3, 2, 2, 2, 2],
                        first_close=[3, 3, 2, 2, NEVER, NEVER], close_samples=[1, 1, 2, 2, 0, 0],
                        first_out=[NEVER, NEVER, NEVER, NEVER, 3, 0]),
            bodies_record=dict(rows=6, sources=6, samples=6, min_row=0, min_source=1, min_sample=3, min_d2=1.0, close_rows=4,
                               close_row_samples=6, first_close_sample=2, out_rows=2, first_out_sample=0, isolated_rows=0),
            tracers=dict(min_d2=[1, 100, 1.25], min_index=[1, 4, 3], min_sample=[3, 0, 2], first_close=[3, NEVER, 2],
                         close_samples=[1, 0, 2], first_out=[NEVER, 3, NEVER]),
            tracers_record=dict(rows=3, sources=6, samples=6, min_row=0, min_source=1, min_sample=3, min_d2=1.0, close_rows=2,
                                close_row_samples=3, first_close_sample=2, out_rows=1, first_out_sample=3, isolated_rows=0))


def hand_world(dtype):
    """-> (pos, vel, tpos, tvel) of HAND in dtype."""
    return tuple(np.array(HAND[name], dtype) for name in ("pos", "vel", "tpos", "tvel"))


def hand_expected(which, dtype):
    """HAND's stated numbers as (record, rows dict) in the dtypes of the contract; which: "bodies" or "tracers"."""
    want = HAND[which]
    rows = {"min_d2": np.array(want["min_d2"], dtype), "min_index": np.array(want["min_index"], np.int32)}
    rows.update({name: np.array(want[name], np.uint32) for name in ROWS[2:]})
    rec = np.zeros(1, DTYPE)[0]
    for name, v in HAND[which + "_record"].items():
        rec[name] = v
    return rec, rows


LATTICE_N = 257       # a lattice world that stands still (weight 0, velocity 0): every sample repeats the first, so every target's
#                       minimum is tied over all samples, and most have two to four sources tied within a sample


def static_lattice(dtype):
    """-> (pos, vel): the scene's lattice world (kind 1) at rest."""
    pos = S.world(S.seed_of("watch", "lattice"), 1, LATTICE_N, dtype)
    return pos, np.zeros_like(pos)
