"""An independent NumPy restatement of the summary contract (include/nbody_ensemble.h, "summaries of an ensemble"): one segment's
record from its rows, written from the header's text and sharing no code with the library.  Every elementwise NumPy operation
on float64 arrays is one IEEE double operation (NumPy fuses nothing), so the grouping written here is the grouping computed.

`record(...)` is the contract.  `ordered_sum(...)` alone is the order of the six ordered sums, with switches that turn it into
the rivals the host test compares against: an ascending-row sequential sum (`sequential`), a 64-chain version (chains=64: chain
l adds rows l + 64 i, i = 0 .. 63, then strides 32 .. 1) and chunks combined by a stride tree instead of in ascending order
(`chunk_tree`)."""
import numpy as np

CHUNK = 4096

DTYPE = np.dtype([(name, "<i8") for name in ("rows", "counted", "in_bounds", "sep_rows")] +
                 [(name, "<f8") for name in ("mass", "min_x", "min_y", "max_x", "max_y", "max_speed2", "sum_wx", "sum_wy", "sum_wvx",
                                             "sum_wvy", "sum_wv2", "sep_max2", "sep_sum2")])
ORDERED = ("sum_wx", "sum_wy", "sum_wvx", "sum_wvy", "sum_wv2", "sep_sum2")


def _chunk_value(t, chains):
    """t: the CHUNK terms of a chunk (+0.0 where a row adds nothing) -> P[0]."""
    acc = np.zeros(chains)
    for row in t.reshape(CHUNK // chains, chains):     # row i holds the terms of rows l + chains * i
        acc = acc + row
    s = chains // 2
    while s >= 1:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s //= 2
    return acc[0]


def ordered_sum(terms, chains=256, sequential=False, chunk_tree=False):
    """terms: float64[rows], +0.0 where a row does not contribute (a chain from +0.0 never holds -0.0, so adding +0.0 and adding
    nothing give the same bits)."""
    terms = np.asarray(terms, np.float64)
    with np.errstate(all="ignore"):
        if sequential:
            acc = np.float64(0.0)
            for t in terms:
                acc = acc + t
            return acc
        n_chunks = max(1, -(-len(terms) // CHUNK))
        padded = np.zeros(n_chunks * CHUNK)
        padded[:len(terms)] = terms
        values = [_chunk_value(padded[c * CHUNK:(c + 1) * CHUNK], chains) for c in range(n_chunks)]
        if chunk_tree:                                 # the chunk's own tree over the chunks: P[c] + P[c + s], s = .., 2, 1
            size = 1
            while size < n_chunks:
                size *= 2
            p = np.zeros(size)
            p[:n_chunks] = values
            s = size // 2
            while s >= 1:
                p[:s] = p[:s] + p[s:2 * s]
                s //= 2
            return p[0]
        acc = values[0]
        for v in values[1:]:
            acc = acc + v
        return acc


def _least(v):
    """The minimum by value with -0.0 below +0.0; +inf of nothing."""
    if not len(v):
        return np.float64(np.inf)
    m = v.min()
    return np.float64(-0.0) if m == 0 and np.signbit(v[v == 0]).any() else (np.float64(0.0) if m == 0 else m)


def _most(v, of_nothing=-np.inf):
    if not len(v):
        return np.float64(of_nothing)
    m = v.max()
    return np.float64(0.0) if m == 0 and not np.signbit(v[v == 0]).all() else (np.float64(-0.0) if m == 0 else m)


def terms(pos, vel, weight=None, ref=None):
    """-> (counted mask, in both mask, {ordered field: float64[rows] of its terms, +0.0 where the row adds nothing}, w, v2, d2)."""
    f32 = pos.dtype == np.float32
    x, y, vx, vy = (a.astype(np.float64) for a in (pos[:, 0], pos[:, 1], vel[:, 0], vel[:, 1]))
    n = len(x)
    if weight is None:
        w = np.ones(n)
    else:
        w = (weight.astype(np.float32) if f32 else weight).astype(np.float64)
    counted = np.isfinite(x) & np.isfinite(y) & np.isfinite(vx) & np.isfinite(vy)
    with np.errstate(all="ignore"):
        v2 = vx * vx + vy * vy
        t = {"sum_wx": w * x, "sum_wy": w * y, "sum_wvx": w * vx, "sum_wvy": w * vy, "sum_wv2": w * v2}
        both = np.zeros(n, bool)
        d2 = np.zeros(n)
        if ref is not None:
            rx, ry, rvx, rvy = (a.astype(np.float64) for a in (ref[0][:, 0], ref[0][:, 1], ref[1][:, 0], ref[1][:, 1]))
            both = counted & np.isfinite(rx) & np.isfinite(ry) & np.isfinite(rvx) & np.isfinite(rvy)
            dx, dy = x - rx, y - ry
            d2 = dx * dx + dy * dy
    out = {k: np.where(counted, v, 0.0) for k, v in t.items()}
    out["sep_sum2"] = np.where(both, d2, 0.0)
    return counted, both, out, w, v2, d2


def record(pos, vel, weight=None, ref=None, height=0, **order):
    """pos, vel [rows, 2] float32 or float64; weight uint32[rows] or None (all 1); ref None or (position, velocity) of the
    reference world's rows -> DTYPE scalar.  order: ordered_sum's switches (none: the contract)."""
    x, y = pos[:, 0].astype(np.float64), pos[:, 1].astype(np.float64)
    counted, both, t, w, v2, d2 = terms(pos, vel, weight, ref)
    r = np.zeros(1, DTYPE)[0]
    r["rows"] = len(x)
    r["counted"] = int(counted.sum())
    h = np.float64(height)
    r["in_bounds"] = int(((y < h) & (x < h) & (y >= 0) & (x >= 0)).sum())
    r["sep_rows"] = int(both.sum())
    r["mass"] = float(sum(int(v) for v in w[counted]))          # integers: exact in any order
    r["min_x"], r["min_y"] = _least(x[counted]), _least(y[counted])
    r["max_x"], r["max_y"] = _most(x[counted]), _most(y[counted])
    r["max_speed2"] = _most(v2[counted], 0.0)
    r["sep_max2"] = _most(d2[both], 0.0)
    for name in ORDERED:
        r[name] = ordered_sum(t[name], **order)
    return r


def same(a, b):
    """Two records (or arrays of records) bit for bit, a NaN field matching any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype.itemsize != b.dtype.itemsize:
        return False
    for name in DTYPE.names:
        u, v = a[name], b[name]
        if DTYPE[name].kind == "f":
            nan = np.isnan(u) & np.isnan(v)
            if not np.array_equal(np.where(nan, 0, u.view(np.int64)), np.where(nan, 0, v.view(np.int64))):
                return False
        elif not np.array_equal(u, v):
            return False
    return True


def diff(a, b):
    """The names of the fields in which two records differ (for messages)."""
    return [name for name in DTYPE.names if not same(only(a, name), only(b, name))]


def only(a, name):
    """The record(s) with every field but `name` zeroed."""
    r = np.zeros(np.asarray(a).shape, DTYPE)
    r[name] = np.asarray(a)[name]
    return r
