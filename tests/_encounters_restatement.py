"""The encounters' contract (include/nbody_ensemble.h, "encounters of an ensemble") restated in NumPy, independently of the
library: elementwise float32 / float64 arithmetic over all targets at once, one source after another in ascending order, ties
handled by explicit comparisons (no argmin).  `rows` gives the per-target arrays, `record` the world's record from them,
`segment` both.  Two rivals for the host tests: `highest=True` keeps the highest source index of a tie, `fused=True` computes
d2 as fma(dy, dy, dx*dx) would (to within a second rounding in rare cases: it only has to show that these rows can tell)."""
import numpy as np

DTYPE = np.dtype([(name, np.int64) for name in ("rows", "sources", "live_pairs", "skipped_pairs", "close_pairs", "close_rows",
                                                "isolated_rows", "min_row", "min_source")] +
                 [("min_d2", np.float64), ("max_nn_row", np.int64), ("max_nn_d2", np.float64)])
CHUNK = 1024          # the kernel's source chunk (kEncounterChunk): the sizes around it are the tests' to visit


def _split(a):
    """Veltkamp: a == hi + lo with 26-bit halves (float64)."""
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def _fused(dx, dy):
    """fma(dy, dy, dx*dx) in the arrays' precision."""
    p = dx * dx
    if dx.dtype == np.float32:
        return (p.astype(np.float64) + dy.astype(np.float64) * dy.astype(np.float64)).astype(np.float32)
    h = dy * dy
    bh, bl = _split(dy)
    e = ((bh * bh - h) + 2.0 * bh * bl) + bl * bl       # dy*dy == h + e
    s = p + h
    v = s - p
    t = (p - (s - v)) + (h - v)                         # p + h == s + t
    out = s + (t + e)
    return np.where(np.isfinite(out), out, p + h)


def rows(targets, sources, own, limit2, highest=False, fused=False):
    """-> (nn_index int32, nn_d2, close uint32, live int64) per target.  own: source j is target j itself, not a pair."""
    T = targets.dtype.type
    n_t, n_s = targets.shape[0], sources.shape[0]
    tx, ty = targets[:, 0].copy(), targets[:, 1].copy()
    idx = np.full(n_t, -1, np.int32)
    best = np.full(n_t, np.inf, T)
    close = np.zeros(n_t, np.uint32)
    live = np.zeros(n_t, np.int64)
    tiny = np.finfo(T).tiny
    limit = T(limit2)
    with np.errstate(all="ignore"):
        for j in range(n_s):
            dx = sources[j, 0] - tx
            dy = sources[j, 1] - ty
            s = np.abs(dx) + np.abs(dy)
            d2 = _fused(dx, dy) if fused else dx * dx + dy * dy
            ok = np.isfinite(s) & (s >= tiny)                        # a normal number
            if own:
                ok[j] = False
            live += ok
            close += (ok & (d2 < limit)).astype(np.uint32)
            take = ok & ((idx < 0) | ((d2 <= best) if highest else (d2 < best)))
            best = np.where(take, d2, best)
            idx = np.where(take, np.int32(j), idx)
    assert best.dtype == targets.dtype
    return idx, best, close, live


def record(n_sources, own, idx, best, close, live):
    r = np.zeros(1, DTYPE)[0]
    n_t = idx.shape[0]
    r["rows"], r["sources"] = n_t, n_sources
    r["live_pairs"] = int(live.sum())
    r["skipped_pairs"] = n_t * (n_sources - (1 if own else 0)) - int(live.sum())
    r["close_pairs"] = int(close.astype(np.int64).sum())
    r["close_rows"] = int((close > 0).sum())
    r["isolated_rows"] = int((idx < 0).sum())
    r["min_row"] = r["min_source"] = r["max_nn_row"] = -1
    r["min_d2"], r["max_nn_d2"] = np.inf, 0.0
    for i in np.flatnonzero(idx >= 0):                               # ascending: a strict comparison keeps the lowest row
        d = float(best[i])
        if r["min_row"] < 0 or d < r["min_d2"]:
            r["min_row"], r["min_source"], r["min_d2"] = i, idx[i], d
        if r["max_nn_row"] < 0 or d > r["max_nn_d2"]:
            r["max_nn_row"], r["max_nn_d2"] = i, d
    return r


def segment(targets, sources=None, limit2=0.0, **rival):
    """-> (record, nn_index, nn_d2, close) of one segment; sources None: the targets are the world's bodies."""
    own = sources is None
    src = targets if own else sources
    idx, best, close, live = rows(targets, src, own, limit2, **rival)
    return record(src.shape[0], own, idx, best, close, live), idx, best, close


def same(a, b):
    """Bit for bit: records, or arrays of one dtype and shape."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_segment(got, want):
    return all(same(g, w) for g, w in zip(got, want)) and len(got) == len(want) == 4


def diff(got, want):
    """The names of what differs between two segments, for a failure message."""
    out = [f for f in DTYPE.names if not same(got[0][f], want[0][f])]
    out += [name for name, g, w in zip(("nn_index", "nn_d2", "close"), got[1:], want[1:]) if not same(g, w)]
    return out
