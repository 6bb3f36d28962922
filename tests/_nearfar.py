"""The near/far split of the direct step (csrc/nearfar.hip) restated in numpy, and scenes that pin it at its cell edges.

The rule: on a grid of pitch h = sqrt(clamp) * 1.001 a body is NEAR when another body lies in its own cell or one of the 8 around
it (or when its mass is not `heavy_base`, where one is given); everything else is FAR and is summed without the clamp.  The
device reaches the same answer through hashed 2 x 2 super-cells, four lookups and four parity-dependent masks; nothing of that
is repeated here.  cell() uses the device's own double operations, so it reproduces bit for bit.

Scenes are built by CELL INDEX AND FRACTION, x = float32((cx + fx) * h), and every builder asserts from cell() that the rounding
to f32 left each body in the cell it was meant for."""
import numpy as np

F32 = np.float32
CLAMP = 0.001
CELL_BIAS = 1 << 29
FAR_POINT = F32(1e30)
FAST_BIG = F32(2.0 ** 60)
FAST_TINY = F32(2.0 ** -22)
NEIGHBOURHOOD = [(dx, dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1)]          # (0, 0): the body's own cell
CASES = [(px, py, dx, dy) for px in (0, 1) for py in (0, 1) for dx, dy in NEIGHBOURHOOD]   # the 36 (parity, cell) cases


# ---------------------------------------------------------------------------------------------------- the rule
def pitch(clamp=CLAMP):
    h = np.sqrt(np.float64(F32(clamp))) * 1.001
    return h, 1.0 / h


def cell(pos, clamp=CLAMP):
    """floor(float64(x) * inv_h) per coordinate, as float64 (NaN and inf stay what they are)."""
    with np.errstate(invalid="ignore"):
        return np.floor(np.asarray(pos, F32).astype(np.float64) * pitch(clamp)[1])


def in_range(c):
    """Per body: both cell coordinates strictly between -2^29 + 2 and 2^29 - 2 (a NaN is not)."""
    with np.errstate(invalid="ignore"):
        return np.all((c > -CELL_BIAS + 2) & (c < CELL_BIAS - 2), axis=-1)


def near(pos, mass=None, heavy_base=0.0, clamp=CLAMP, skip=None):
    """near[i]: another body lies in the 3 x 3 cells around body i, or mass[i] != heavy_base when heavy_base > 0.
    Bodies outside the grid's range take no part (the device falls back to one clamped pass then: their sets are not compared).
    skip = (px, py, dx, dy): the rule with ONE cell deleted, for bodies whose cell has that parity (the coverage proof)."""
    pos = np.asarray(pos, F32).reshape(-1, 2)
    c = cell(pos, clamp)
    ok = in_range(c)
    ci = np.where(ok[:, None], c, 0.0).astype(np.int64)

    def key(cx, cy):
        return (cx + CELL_BIAS) * (1 << 31) + (cy + CELL_BIAS)

    keys, counts = np.unique(key(ci[ok, 0], ci[ok, 1]), return_counts=True)
    out = np.zeros(len(pos), bool)
    for dx, dy in NEIGHBOURHOOD:
        if len(keys) == 0:
            break
        k = key(ci[:, 0] + dx, ci[:, 1] + dy)
        at = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
        bodies = np.where(keys[at] == k, counts[at], 0)
        hit = bodies >= (2 if (dx, dy) == (0, 0) else 1)
        if skip is not None and (dx, dy) == tuple(skip[2:]):
            hit &= ~(((ci[:, 0] & 1) == skip[0]) & ((ci[:, 1] & 1) == skip[1]))
        out |= hit
    out &= ok
    if heavy_base > 0:
        out |= np.asarray(mass, F32) != F32(heavy_base)
    return out


def outside_fast(pos):
    """FAST's domain as nf_insert and direct_hazard_scan spell it: finite, below 2^60, and zero or at least 2^-22."""
    with np.errstate(invalid="ignore"):
        a = np.abs(np.asarray(pos, F32))
        return ~(a < FAST_BIG) | ((a != 0) & (a < FAST_TINY))


def expected_flags(pos, is_near, use_hazard, clamp=CLAMP):
    """(hazard, fallback, n_near, state) as the split leaves them."""
    pos = np.asarray(pos, F32).reshape(-1, 2)
    n = len(pos)
    hazard = bool(use_hazard and outside_fast(pos).any())
    fallback = bool((~in_range(cell(pos, clamp))).any())
    n_near = int(np.count_nonzero(is_near))
    state = 2 if hazard else (1 if fallback or n_near > n // 64 else 0)
    return int(hazard), int(fallback), n_near, state


def far_padded(n):
    return (n + 15) // 16 * 16


def expected_far(pos, is_near, couples):
    """The far copy: the positions bit for bit, the far-away point in every near slot and, in couples, in every slot from n to
    far_padded(n); couples order is {xA, xB, yA, yB} per two slots.  Returns the flat floats (couples) or (n, 2)."""
    pos = np.asarray(pos, F32).reshape(-1, 2)
    n = len(pos)
    slots = far_padded(n) if couples else n
    far = np.full((slots, 2), FAR_POINT, F32)
    far[:n] = pos
    far[:n][is_near] = FAR_POINT
    return far.reshape(slots // 2, 2, 2).transpose(0, 2, 1).reshape(-1).copy() if couples else far


def expected_minv(mass):
    with np.errstate(divide="ignore"):
        return F32(1) / np.asarray(mass, F32)          # IEEE; a zero mass gives inf


# ---------------------------------------------------------------------------------------------------- scenes
def place(cells, fracs, clamp=CLAMP):
    """Bodies at (cell + fraction) * h in f32; asserts that every body landed in its cell."""
    cells = np.asarray(cells, np.int64).reshape(-1, 2)
    fracs = np.asarray(fracs, np.float64).reshape(-1, 2)
    pos = ((cells + fracs) * pitch(clamp)[0]).astype(F32)
    assert np.array_equal(cell(pos, clamp), cells.astype(np.float64)), "f32 rounding moved a body out of its cell"
    return pos


def lattice(m, base=(20000, 20000), step=8):
    """m single bodies on a lattice of pitch `step` cells (row-major in a square), each in the middle of its cell: all far."""
    side = int(np.ceil(np.sqrt(m)))
    k = np.arange(m)
    cells = np.stack([base[0] + step * (k % side), base[1] + step * (k // side)], axis=1)
    return place(cells, np.full((m, 2), 0.5))


BASES = [(1000, 1000), (-3000, 1000), (1000, -3000), (-3000, -3000)]


def _pair(anchor, d):
    """An anchor and its partner `d` cells away, pushed towards each other (fractions 0.5 +- 0.4 sign(d)); in one cell 0.4 h apart."""
    d = np.asarray(d)
    s = np.sign(d)
    fa, fb = 0.5 + 0.4 * s, 0.5 - 0.4 * s
    if not d.any():
        fa, fb = np.array([0.3, 0.5]), np.array([0.7, 0.5])
    return [tuple(anchor), tuple(np.asarray(anchor) + d)], [tuple(fa), tuple(fb)]


def planted_pairs():
    """-> (cells, fracs, pairs): pairs[k] = (row of the anchor, row of the partner, (px, py), (dx, dy)).
    Main part: around each of BASES, every anchor parity x every partner offset in [-2, 2]^2, anchors 16 cells apart.
    Across the axes: pairs whose cells are -1 and 0 in x (and the same in y), anchored on either side, both parities of the other
    coordinate, the partner one cell down, level and one cell up."""
    cells, fracs, pairs = [], [], []

    def add(anchor, d):
        c, f = _pair(anchor, d)
        pairs.append((len(cells), len(cells) + 1, (anchor[0] & 1, anchor[1] & 1), tuple(d)))
        cells.extend(c)
        fracs.extend(f)

    offsets = [(dx, dy) for dx in range(-2, 3) for dy in range(-2, 3)]
    for bx, by in BASES:
        k = 0
        for px in (0, 1):
            for py in (0, 1):
                for d in offsets:
                    add((bx + 16 * (k % 10) + px, by + 16 * (k // 10) + py), d)
                    k += 1
    k = 0
    for axis in (0, 1):
        for side in (-1, 0):
            for q in (0, 1):
                for d_other in (-1, 0, 1):
                    anchor, d = [0, 0], [0, 0]
                    anchor[axis], d[axis] = side, (1 if side == -1 else -1)
                    anchor[1 - axis], d[1 - axis] = 200 + 16 * k + q, d_other
                    add(tuple(anchor), tuple(d))
                    k += 1
    return np.array(cells, np.int64), np.array(fracs), pairs


N_SCENE = 24576          # 336 near bodies need n // 64 >= 336 for state 0: 20 480 gives 320 and falls back, 24 576 gives 384


def planted_scene(n=N_SCENE, seed=1):
    """The planted pairs among lattice singles, rows shuffled by `seed` (so the near bodies are spread over the work-groups).
    -> (pos, pairs) with the pairs' rows in the shuffled order."""
    cells, fracs, pairs = planted_pairs()
    pos = np.concatenate([place(cells, fracs), lattice(n - len(cells))])
    where = np.random.default_rng(seed).permutation(n)          # body k of the construction is row where[k]
    out = np.empty_like(pos)
    out[where] = pos
    return out, [(int(where[a]), int(where[b]), par, d) for a, b, par, d in pairs]


def counted_scene(n_near, n=N_SCENE, seed=2):
    """Lattice singles plus same-cell pairs (0.4 h apart), and one triple where n_near is odd: exactly n_near near bodies.
    n_near = 1 has no geometry: the scene is all singles, and the caller makes one body's mass odd."""
    assert n_near >= 0 and n_near != 1
    cells, fracs = [], []
    groups = [2] * (n_near // 2 - (n_near & 1)) + ([3] if n_near & 1 else [])
    for k, g in enumerate(groups):
        c = (1000 + 16 * (k % 14) + (k & 1), -3000 + 16 * (k // 14) + ((k >> 1) & 1))
        cells.extend([c] * g)
        fracs.extend([(0.3, 0.5), (0.7, 0.5), (0.5, 0.8)][:g])
    planted = place(cells, fracs) if cells else np.zeros((0, 2), F32)
    pos = np.concatenate([planted, lattice(n - len(planted))])
    where = np.random.default_rng(seed).permutation(n)
    out = np.empty_like(pos)
    out[where] = pos
    return out


def range_edge(sign, clamp=CLAMP):
    """The f32 coordinates on either side of the grid's range edge at that sign: (last in range, first out of range)."""
    x = F32(sign * (CELL_BIAS - 2) * pitch(clamp)[0])
    toward_zero, away = F32(0), F32(sign * np.inf)
    while not in_range(cell([[x, 0]], clamp))[0]:
        x = np.nextafter(x, toward_zero)
    while in_range(cell([[np.nextafter(x, away), 0]], clamp))[0]:
        x = np.nextafter(x, away)
    return x, np.nextafter(x, away)


FAST_EDGE_VALUES = [v for m in (FAST_BIG, np.nextafter(FAST_BIG, F32(0)), FAST_TINY, np.nextafter(FAST_TINY, F32(0))) for v in (m, -m)] + [
    np.nextafter(F32(0), F32(1)), F32(-0.0), F32(0.0), F32(np.inf), F32(np.nan)]
