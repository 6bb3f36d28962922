"""Scenes for the edges of the device quad-tree build (quad_build.hip, quad_build_device in tree_build_driver.hip), shared by
test_quad_edge_scenes_host.py (no GPU: are the scenes what the GPU tests assume?) and test_gpu_quad_build_edges.py.

Every scene is seeded and a function of its arguments only: the same call gives the same rows.  Every root cell is exactly
representable in f32 (Params.quad_root_* are floats; the oracle takes the same values).  Families:
  A  exact(D): nine points that put one leaf at depth exactly D, first or last in tree order (the 31 child codes of the
     path key, the sort depth, the ends of the 17-key window of qb_leaf_order);
  B  siblings_full(D): two full leaves under one parent, side by side in key order;
  C  midline_lattice: every coordinate is a cell border (the strict `>` of qb_path_keys);
  D  special values: NaN, infinities, signed zeros, subnormals, huge coordinates;
  E  masses: full-range u32 weights, node masses that wrap to exactly 0, zero weights;
  F  roots: a centred root, a root at (-0.0, -0.0), a root far smaller than the cloud;
  G  collapse: forty bodies that meet in a tiny box after one step and part again (the re-sort inside one call)."""
import numpy as np

ROOT = (0.0, 0.0, 100000.0)                     # the library's default root cell
KEYS = ("mass", "is_leaf", "first", "count", "skip", "order")


def _f64(dtype):
    return np.dtype(dtype) == np.float64


def weights(n):
    return (np.arange(n) % 7 + 1).astype(np.uint32)


def background(rng, n):
    """n rows drawn uniformly from [2e4, 8e4)^2, in f64."""
    return 2e4 + rng.random((n, 2)) * 6e4


def uniform(dtype, n, seed=0):
    """n uniform rows over the default root cell (n <= 8: the root is a leaf)."""
    rng = np.random.default_rng(7000 + 16 * n + seed)
    return (rng.random((n, 2)) * 1e5).astype(dtype), weights(n)


# ---------------------------------------------------------------- shared comparison
def tree_equal_bits(t, o, tag=None):
    """t: a tree_export() / host_tree() dict; o: the oracle's FlatQuad.  The index arrays are equal, geom has the oracle's
    NaN mask, and every entry of geom that is not NaN has the oracle's bits (so +0.0 is not -0.0).  The sign and payload of a
    NaN are not compared: they are what the machine's 0/0 gives, and no part of the contract."""
    for k in KEYS:
        assert np.array_equal(t[k], getattr(o, k)), (tag, k)
    g, r = np.ascontiguousarray(t["geom"]), np.ascontiguousarray(o.geom)
    assert g.dtype == r.dtype and g.shape == r.shape, (tag, g.dtype, r.dtype, g.shape, r.shape)
    gn, rn = np.isnan(g), np.isnan(r)
    assert np.array_equal(gn, rn), (tag, "NaN mask", np.argwhere(gn != rn)[:4].tolist())
    u = np.uint64 if g.dtype == np.float64 else np.uint32
    gb, rb = g.view(u), r.view(u)
    bad = (gb != rb) & ~rn
    assert not bad.any(), (tag, "geom bits", np.argwhere(bad)[:4].tolist(), g[bad][:4].tolist(), r[bad][:4].tolist())


# ---------------------------------------------------------------- A
EXACT_OFFSETS = np.array([(0.1, 0.1), (0.2, 0.3), (0.3, 0.2), (0.4, 0.4), (0.15, 0.35),
                          (1.1, 1.2), (1.3, 1.4), (1.5, 1.6), (1.7, 1.8)])
EXACT_SIZES = (9, 16, 17, 255, 256, 257, 300)
EXACT_MAX_D = {"sw": 33, "ne": 20}             # f32 cannot resolve a deeper cell next to 1e5


def exact(dtype, D, n=300, corner="sw"):
    """-> (pos[n, 2], weight[n], rows): five points in the depth-D cell at the root's south-west corner (at 1e5 - p: its
    north-east corner) and four in that cell's diagonal sibling: the nine share a depth-(D-1) cell, so it splits, and the
    deepest leaf lies at depth exactly D.  They stand in the middle of n - 9 background rows; `rows` are their indices.
    They are the first nine rows of the tree order (sw) or the last nine (ne)."""
    assert corner in ("sw", "ne") and n >= 9
    rng = np.random.default_rng(1000 + 64 * D + (32 if corner == "ne" else 0) + n % 31)
    p = EXACT_OFFSETS * (1e5 / 2.0 ** D)
    if corner == "ne":
        p = 1e5 - p
    bg = background(rng, n - 9)
    at = (n - 9) // 2
    pos = np.concatenate([bg[:at], p, bg[at:]]).astype(dtype)
    return np.ascontiguousarray(pos), weights(n), np.arange(at, at + 9)


# ---------------------------------------------------------------- B
def siblings_cell(D):
    """(x, y, c): origin and height of the first of the two depth-D sibling cells of siblings_full (the second lies at x + c).
    Their parent lies near (0.1, 0.85) of the root cell: away from the corners and outside the background's box."""
    c = 1e5 / 2.0 ** D
    ix, iy = int(0.1 * 2 ** (D - 1)), int(0.85 * 2 ** (D - 1))
    return ix * 2 * c, iy * 2 * c, c


def siblings_full(dtype, D, n=300):
    """-> (pos, weight, rows_a, rows_b): eight points in one depth-D cell (rows_a) and eight in its sibling to the east
    (rows_b), scattered among n - 16 background rows: two full leaves under one parent, adjacent in key order."""
    rng = np.random.default_rng(2000 + D)
    x, y, c = siblings_cell(D)
    a = np.array([x, y]) + (0.1 + 0.8 * rng.random((8, 2))) * c
    b = np.array([x + c, y]) + (0.1 + 0.8 * rng.random((8, 2))) * c
    pos = np.concatenate([a, b, background(rng, n - 16)])
    perm = rng.permutation(n)
    pos = np.ascontiguousarray(pos[perm].astype(dtype))
    where = np.argsort(perm)                         # where[j]: the row that holds the j-th row made above
    return pos, weights(n), np.sort(where[:8]), np.sort(where[8:16])


# ---------------------------------------------------------------- C
LATTICE_ROOTS = ((0.0, 0.0, 1e5), (-5e4, -5e4, 2e5))
LATTICE_STEP = 1562.5


def midline_lattice(dtype, root=LATTICE_ROOTS[0]):
    """The 64 x 64 lattice on the multiples of 1562.5, rows shuffled: under either root of LATTICE_ROOTS every coordinate is
    the border of a cell of some level <= 7, so every point sits on a midline on its way down."""
    assert tuple(root) in LATTICE_ROOTS
    k = np.arange(64) * LATTICE_STEP
    pos = np.stack(np.meshgrid(k, k, indexing="ij"), axis=-1).reshape(-1, 2)
    rng = np.random.default_rng(3000 + LATTICE_ROOTS.index(tuple(root)))
    pos = np.ascontiguousarray(pos[rng.permutation(4096)].astype(dtype))
    return pos, weights(4096)


# ---------------------------------------------------------------- D
SPECIAL_NAMES = ("nan_single", "nan_leaf", "inf_single", "zeros_subnormals", "huge", "nan_nine")
SPECIAL_N = 500


def special(name, dtype):
    """-> (pos[500, 2], weight[500]): uniform rows over the default root cell with a few replaced."""
    f64 = _f64(dtype)
    n = SPECIAL_N
    rng = np.random.default_rng(4000 + 2 * SPECIAL_NAMES.index(name) + (1 if f64 else 0))
    pos = (rng.random((n, 2)) * 1e5).astype(dtype)
    nan, inf = np.nan, np.inf
    if name == "nan_single":          # a NaN compares false: the row keeps to the west (south) edge and descends by the other
        pos[10:13, 0] = nan
        pos[200:203, 1] = nan
        pos[499, 0] = nan
    elif name == "nan_leaf":          # eight rows that take child 0 at every level: one full leaf at the south-west corner
        pos[60:480:60] = nan
        pos[0] = nan
        assert np.isnan(pos).all(axis=1).sum() == 8
    elif name == "inf_single":
        pos[10, 0] = inf
        pos[11, 1] = inf
        pos[250, 0] = -inf
        pos[251, 1] = -inf
        pos[499] = -inf
    elif name == "zeros_subnormals":  # six rows that never leave the south-west corner; zeros and subnormals along the edges
        sub = 1e-310 if f64 else 1e-40
        pos[5] = (0.0, 0.0)
        pos[6] = (-0.0, -0.0)
        pos[7] = (-0.0, 0.0)
        pos[300] = (sub, sub)
        pos[301] = (sub / 8, -0.0)
        pos[302] = (0.0, sub)
        pos[100::97, 0] = -0.0
        pos[101::97, 1] = 0.0
        pos[102::97, 0] = sub
    elif name == "huge":              # two rows beyond the same corner share a leaf: its sum overflows
        big = 1.7e308 if f64 else 3e38
        pos[10] = (big, big)
        pos[400] = (big, big)
        pos[11] = (-big, -big)
        pos[401] = (-big, -big)
        pos[12, 0] = big
        pos[13, 1] = -big
        pos[14] = (-big, big)
    elif name == "nan_nine":          # one more than a leaf holds: no depth separates them
        pos[50:500:50] = nan
        assert np.isnan(pos).all(axis=1).sum() == 9
    else:
        raise KeyError(name)
    return pos, weights(n)


# ---------------------------------------------------------------- E
MASS_NAMES = ("full_range", "wrap_to_zero", "all_zero")


def masses(name, n):
    if name == "full_range":
        rng = np.random.default_rng(5000 + n % 97)
        return rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    if name == "wrap_to_zero":        # two, four, six or eight heavy rows sum to exactly 0 (mod 2^32)
        w = np.zeros(n, np.uint32)
        w[0::2] = 1 << 31
        return w
    if name == "all_zero":
        return np.zeros(n, np.uint32)
    raise KeyError(name)


# ---------------------------------------------------------------- F
ROOT_NAMES = ("centred", "neg_zero", "small")


def roots(name, dtype):
    """-> (pos, weight, root)."""
    rng = np.random.default_rng(6000 + ROOT_NAMES.index(name))
    n = 500
    if name == "centred":
        pos = rng.random((n, 2)) * 1e5 - 5e4
        root = (-5e4, -5e4, 1e5)
    elif name == "neg_zero":          # -0.0 stays -0.0 down the chain of first children only (quad_tree.rs:183)
        pos = rng.random((n, 2)) * 64.0
        root = (-0.0, -0.0, 64.0)
    elif name == "small":             # most rows outside the root cell; at most eight beyond any one corner
        # a cross through the root cell: rows beyond an edge keep to that edge's cells and part by the other coordinate
        pos = rng.random((n, 2)) * 1024.0 + 3e4
        pos[0:440:2, 0] = rng.random(220) * 1e5
        pos[1:440:2, 1] = rng.random(220) * 1e5
        out = np.array([(-1.0, -2.0), (-3e4, -1.0), (-5.0, -7e4), (2e5, -4.0), (1.5e5, -9e4), (-6.0, 3e5), (-2e4, 1.2e5),
                        (1.1e5, 1.3e5), (4e5, 1.01e5), (1.2e5, 9e5), (2e5, 2e5), (-8.0, 4e4), (5e4, -3.0), (1.4e5, 6e4),
                        (4e4, 1.6e5)])                 # beyond the corners: three or four each
        pos = np.concatenate([pos[:100], out[:8], pos[100:400], out[8:], pos[400:]])
        root = (3e4, 3e4, 1024.0)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(pos.astype(dtype)), weights(pos.shape[0]), root


# ---------------------------------------------------------------- G
COLLAPSE_DELTA = 0.1
COLLAPSE_CENTRE = (51234.5, 49876.25)
COLLAPSE_BOX = 0.01
COLLAPSE_DEEP_BOX = 2e-6


def _collapse(dtype, box, seed):
    rng = np.random.default_rng(seed)
    n = 400
    pos = background(rng, n).astype(dtype)
    vel = np.zeros_like(pos)
    who = np.arange(5, n, 10)                        # forty rows
    land = np.array(COLLAPSE_CENTRE) + (rng.random((who.size, 2)) - 0.5) * box
    vel[who] = ((land - pos[who].astype(np.float64)) / COLLAPSE_DELTA).astype(dtype)
    return pos, vel, np.ones(n, np.uint32), who


def collapse(dtype):
    """-> (pos, vel, weight, rows): 400 bodies in [2e4, 8e4)^2; forty of them (`rows`) land, after one step of 0.1, inside a
    box 0.01 wide near (51234.5, 49876.25) and fly apart in the next: tree depths 5, 25, 5, 5 over three steps."""
    return _collapse(dtype, COLLAPSE_BOX, 8000 + (1 if _f64(dtype) else 0))


def collapse_deep():
    """f64 only: the landing box is 2e-6 wide, so the tree after the first step is deeper than the 31 levels of the device's
    path key (and no deeper than 10 before and after)."""
    return _collapse(np.float64, COLLAPSE_DEEP_BOX, 8100)
