"""The scenes of tests/_quad_edge_scenes.py are what test_gpu_quad_build_edges.py assumes, and the host builder, on which
every declined device build falls back, builds the oracle's tree from each, signed zeros included.  No GPU needed.

A scene that quietly degenerated (a cluster one level shallower than promised, a lattice point that left its midline, a
collapse that never gets deep) would let a GPU test pass for the wrong reason; these checks fail first."""
import numpy as np
import pytest

from tests import _quad_edge_scenes as S

DTYPES = [np.float32, np.float64]
THETA = 0.5


def _check(nb, orc, pos, w, root, tag):
    """No overflow in the oracle; host builder == oracle, bit for bit.  -> the oracle's flat tree."""
    C = nb._capi
    o = orc.Quad(pos, w, root=root).flat()
    assert not o.overflow, tag
    prm = C.default_params()
    prm.quad_root_x, prm.quad_root_y, prm.quad_root_h = root
    h = C.host_tree(C.TREE_QUAD, pos, w, prm)
    assert not h["overflow"], tag
    S.tree_equal_bits(h, o, tag)
    assert h["max_depth"] == int(o.depth.max()), tag
    return o


def test_roots_are_exact_in_f32():
    rs = [S.ROOT, *S.LATTICE_ROOTS] + [S.roots(name, np.float32)[2] for name in S.ROOT_NAMES]
    for r in rs:
        assert all(float(np.float32(v)) == v for v in r), r
    r = S.roots("neg_zero", np.float32)[2]
    assert np.signbit(r[0]) and np.signbit(r[1]) and r[0] == 0 and r[1] == 0


def test_scenes_are_functions_of_their_arguments():
    for a, b in ((S.exact(np.float32, 12, 257, "ne"), S.exact(np.float32, 12, 257, "ne")),
                 (S.siblings_full(np.float64, 6), S.siblings_full(np.float64, 6)),
                 (S.special("huge", np.float32), S.special("huge", np.float32)),
                 (S.collapse(np.float64), S.collapse(np.float64)), (S.collapse_deep(), S.collapse_deep())):
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)
    assert np.array_equal(S.masses("full_range", 500), S.masses("full_range", 500))


# ---------------------------------------------------------------- A
@pytest.mark.parametrize("corner", ["sw", "ne"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_scenes_have_their_depth_and_their_place(nb, orc, dtype, corner):
    """Depth exactly D (30 and 31 build on the device, 32 and 33 are declined; D + 3 and D + 4 against the depth before), and
    the nine rows first (sw) or last (ne) in tree order: the two ends of the sorted keys."""
    for D in range(6, S.EXACT_MAX_D[corner] + 1):
        for n in S.EXACT_SIZES:
            pos, w, rows = S.exact(dtype, D, n, corner)
            assert pos.dtype == dtype and pos.shape == (n, 2) and rows.shape == (9,)
            o = _check(nb, orc, pos, w, S.ROOT, (corner, D, n))
            assert int(o.depth.max()) == D, (corner, D, n, int(o.depth.max()))
            got = o.order[:9] if corner == "sw" else o.order[-9:]
            assert sorted(got.tolist()) == rows.tolist(), (corner, D, n)
            # the leaves of the nine: five and four points, both at depth D
            deep = np.flatnonzero((o.depth == D) & (o.is_leaf != 0))
            assert sorted(o.count[deep].tolist()) == [4, 5], (corner, D, n)


@pytest.mark.parametrize("dtype", DTYPES)
def test_small_scenes_are_one_leaf(nb, orc, dtype):
    for n in (1, 8):
        pos, w = S.uniform(dtype, n)
        o = _check(nb, orc, pos, w, S.ROOT, n)
        assert o.skip.shape[0] == 1 and o.is_leaf[0] == 1 and o.count[0] == n


# ---------------------------------------------------------------- B
@pytest.mark.parametrize("D", [6, 12])
@pytest.mark.parametrize("dtype", DTYPES)
def test_siblings_are_two_full_leaves_side_by_side(nb, orc, dtype, D):
    pos, w, ra, rb = S.siblings_full(dtype, D)
    o = _check(nb, orc, pos, w, S.ROOT, D)
    full = np.flatnonzero((o.is_leaf != 0) & (o.count == 8) & (o.depth == D))
    assert full.shape[0] == 2 and full[1] == full[0] + 1, full
    a, b = int(full[0]), int(full[1])
    assert o.first[b] == o.first[a] + 8                               # sixteen consecutive places of the tree order
    assert o.order[o.first[a]:o.first[a] + 8].tolist() == ra.tolist()  # in index order inside each leaf
    assert o.order[o.first[b]:o.first[b] + 8].tolist() == rb.tolist()
    assert o.depth[a - 1] == D - 1 and o.is_leaf[a - 1] == 0 and o.skip[a - 1] == b + 1   # one parent, these two children only
    assert not np.array_equal(ra, np.arange(ra[0], ra[0] + 8))          # the rows are scattered


# ---------------------------------------------------------------- C
@pytest.mark.parametrize("root", S.LATTICE_ROOTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_lattice_sits_on_midlines_and_tells_strict_from_not(nb, orc, dtype, root):
    pos, w = S.midline_lattice(dtype, root)
    assert pos.shape == (4096, 2) and np.unique(pos, axis=0).shape[0] == 4096
    k = (pos.astype(np.float64) - root[0]) * 128.0 / root[2]
    assert np.array_equal(k, np.round(k)) and k.min() >= 0 and k.max() < 128       # a border of a level <= 7 cell
    o = _check(nb, orc, pos, w, root, root)
    # one ulp up and every point is on the other side of its midline: `>=` for `>` would build that tree from this scene
    up = np.nextafter(pos, dtype(np.inf))
    o2 = orc.Quad(up, w, root=root).flat()
    assert not o2.overflow
    assert o2.skip.shape[0] != o.skip.shape[0] or not np.array_equal(o2.order, o.order)
    assert not np.array_equal(o2.order, o.order)


# ---------------------------------------------------------------- D
@pytest.mark.parametrize("dtype", DTYPES)
def test_special_scenes_hold_what_their_names_say(dtype):
    f64 = dtype == np.float64
    tiny = np.finfo(dtype).tiny
    p = S.special("nan_single", dtype)[0]
    assert np.isnan(p).any(axis=1).sum() == 7 and not np.isnan(p).all(axis=1).any()
    p = S.special("nan_leaf", dtype)[0]
    assert np.isnan(p).all(axis=1).sum() == 8 and np.isnan(p).sum() == 16
    p = S.special("nan_nine", dtype)[0]
    assert np.isnan(p).all(axis=1).sum() == 9 and np.isnan(p).sum() == 18
    p = S.special("inf_single", dtype)[0]
    assert np.isposinf(p).sum() == 2 and np.isneginf(p).sum() == 4 and np.isneginf(p).all(axis=1).sum() == 1
    p = S.special("zeros_subnormals", dtype)[0]
    zero = p == 0
    assert (zero & np.signbit(p)).sum() >= 5 and (zero & ~np.signbit(p)).sum() >= 5
    assert ((p > 0) & (p < tiny)).sum() >= 5                                     # subnormal, not flushed
    p = S.special("huge", dtype)[0]
    assert np.isfinite(p).all() and np.abs(p).max() == dtype(1.7e308 if f64 else 3e38)
    with np.errstate(over="ignore"):
        assert np.isposinf(p[10, 0] + p[400, 0]) and np.isneginf(p[11, 1] + p[401, 1])
    for name in S.SPECIAL_NAMES:
        p, w = S.special(name, dtype)
        assert p.dtype == dtype and p.shape == (S.SPECIAL_N, 2) and w.shape == (S.SPECIAL_N,)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [s for s in S.SPECIAL_NAMES if s != "nan_nine"])
def test_special_scenes_build_finite_trees(nb, orc, dtype, name):
    pos, w = S.special(name, dtype)
    o = _check(nb, orc, pos, w, S.ROOT, name)
    assert int(o.depth.max()) <= 10
    if name == "nan_leaf":      # the eight rows are one leaf, the first of the tree
        j = int(np.flatnonzero(o.is_leaf != 0)[0])
        assert o.count[j] == 8 and np.isnan(pos[o.order[:8]]).all()
    if name in ("nan_single", "nan_leaf"):
        assert np.isnan(o.geom[0, 3:]).any()                                      # and the NaN reaches the root's centre


@pytest.mark.parametrize("dtype", DTYPES)
def test_nine_nan_rows_overflow_everywhere(nb, orc, dtype):
    C = nb._capi
    pos, w = S.special("nan_nine", dtype)
    assert orc.Quad(pos, w).flat().overflow
    assert C.host_tree(C.TREE_QUAD, pos, w)["overflow"]


# ---------------------------------------------------------------- E
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", S.MASS_NAMES)
def test_mass_scenes(nb, orc, dtype, name):
    for scene in ("uniform", "lattice"):
        pos = S.uniform(dtype, 500)[0] if scene == "uniform" else S.midline_lattice(dtype)[0]
        w = S.masses(name, pos.shape[0])
        assert w.dtype == np.uint32
        o = _check(nb, orc, pos, w, S.ROOT, (name, scene))
        inner = o.is_leaf == 0
        if name == "full_range":
            assert int(w.max()) > 0xF0000000 and int(w.astype(np.uint64).sum()) > 2 ** 32      # the root's mass wraps
            assert int(o.mass[0]) == int(w.astype(np.uint64).sum()) & 0xFFFFFFFF
        else:
            # nodes of mass exactly 0: the centre of an internal one is x / 0: infinite over heavy children whose masses
            # cancel, 0 / 0 = NaN over children without mass (and over a child whose centre is infinite: inf * 0)
            zero = inner & (o.mass == 0)
            assert zero.sum() >= 8, (name, scene, int(zero.sum()))
            assert not np.isfinite(o.geom[zero, 3:]).any()
            nan = zero & np.isnan(o.geom[:, 3:]).all(axis=1)
            assert nan.sum() >= 4, (name, scene, int(nan.sum()))
            if name == "all_zero":
                assert np.array_equal(nan, inner)
        if name == "wrap_to_zero":
            assert (inner & (o.mass != 0)).any() and int(w.astype(np.uint64).sum()) >= 2 ** 32
        if name == "all_zero":
            assert not o.mass.any()


# ---------------------------------------------------------------- F
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", S.ROOT_NAMES)
def test_root_scenes(nb, orc, dtype, name):
    pos, w, root = S.roots(name, dtype)
    o = _check(nb, orc, pos, w, root, name)
    x, y, h = root
    inside = (pos[:, 0] >= x) & (pos[:, 0] < x + h) & (pos[:, 1] >= y) & (pos[:, 1] < y + h)
    if name == "small":
        assert (~inside).sum() > 0.8 * pos.shape[0]
        lo_x, hi_x, lo_y, hi_y = pos[:, 0] < x, pos[:, 0] >= x + h, pos[:, 1] < y, pos[:, 1] >= y + h
        for cx in (lo_x, hi_x):
            for cy in (lo_y, hi_y):
                assert 1 <= (cx & cy).sum() <= 8                                  # beyond one corner: never parted again
    else:
        assert inside.all()
    if name == "neg_zero":
        # -0.0 survives down the chain of first children and nowhere else: `offset + 0.0` anywhere would lose it
        neg = np.signbit(o.geom[:, 0]) & np.signbit(o.geom[:, 1])
        chain = [0]
        while o.is_leaf[chain[-1]] == 0 and o.geom[chain[-1] + 1, 2] == o.geom[chain[-1], 2] / 2 \
                and o.geom[chain[-1] + 1, 0] == 0 and o.geom[chain[-1] + 1, 1] == 0:
            chain.append(chain[-1] + 1)
        assert len(chain) >= 3 and np.flatnonzero(neg).tolist() == chain
        assert np.signbit(o.geom[:, :2]).sum() == 2 * len(chain)
        zero_edge = (o.geom[:, 0] == 0) | (o.geom[:, 1] == 0)
        assert zero_edge.sum() > len(chain)                                       # cells on the axes whose zero is +0.0


# ---------------------------------------------------------------- G
def _depths(orc, pos, vel, w, steps):
    out = []
    for k in range(steps + 1):
        p = pos if k == 0 else orc.update_quad(pos, vel, w, delta=S.COLLAPSE_DELTA, theta=THETA, nsteps=k, nthreads=8)[0]
        o = orc.Quad(p, w).flat()
        assert not o.overflow, k
        out.append(int(o.depth.max()))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_collapse_depths(orc, dtype):
    """5, 25, 5, 5: the second build of the call finds a tree twenty levels deeper than the sort depth it starts with."""
    pos, vel, w, rows = S.collapse(dtype)
    assert pos.shape == (400, 2) and rows.shape == (40,) and pos.dtype == dtype and vel.dtype == dtype
    assert np.count_nonzero(vel.any(axis=1)) == 40
    assert _depths(orc, pos, vel, w, 3) == [5, 25, 5, 5]
    p1 = orc.update_quad(pos, vel, w, delta=S.COLLAPSE_DELTA, theta=THETA, nsteps=1, nthreads=8)[0]
    assert np.abs(p1[rows].astype(np.float64) - np.array(S.COLLAPSE_CENTRE)).max() <= S.COLLAPSE_BOX


def test_collapse_deep_depths(orc):
    """Deeper than the path key's 31 levels after the first step, without overflow; shallow before and after."""
    pos, vel, w, rows = S.collapse_deep()
    assert pos.dtype == np.float64
    d = _depths(orc, pos, vel, w, 3)
    assert d[1] > 31 and d[0] <= 10 and d[2] <= 10 and d[3] <= 10, d
