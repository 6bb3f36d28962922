"""The scenes of tests/_bvh_edge_scenes.py are what test_gpu_bvh_build_edges.py assumes, and the host builder, on which
every declined device build falls back, builds the oracle's tree from each.  No GPU needed.

A scene that quietly degenerated (the reference recursing without end, a group that no longer splits where it should, a
cluster scene that fits the reserve after all) would let a GPU test pass for the wrong reason; these checks fail first."""
import numpy as np
import pytest

from tests import _bvh_edge_scenes as S

DTYPES = [np.float32, np.float64]
KEYS = ("mass", "is_leaf", "first", "count", "skip")


def _check(nb, orc, pos, w, leaf, tag):
    """No overflow in the oracle; host builder == oracle.  -> the oracle's flat tree."""
    C = nb._capi
    o = orc.BVH(pos, w, leaf_size=leaf).flat()
    assert not o.overflow, tag
    prm = C.default_params()
    prm.leaf_size = leaf
    h = C.host_tree(C.TREE_BVH, pos, w, prm)
    assert not h["overflow"], tag
    for k in KEYS:
        assert np.array_equal(h[k], getattr(o, k)), (tag, k)
    assert np.array_equal(h["order"], o.ids), tag
    assert np.array_equal(h["geom"], o.geom, equal_nan=True), tag
    return o


def _points_below(o, node):
    """Points in the subtree of pre-order node `node`."""
    end = int(o.skip[node])
    leaves = o.is_leaf[node:end] != 0
    return int(o.count[node:end][leaves].sum())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", S.SPECIAL_NAMES)
def test_special_value_scenes_build_finite_trees(nb, orc, dtype, name):
    for n in S.SPECIAL_SIZES:
        pos, w = S.special(name, dtype, n)
        assert pos.dtype == dtype and pos.shape == (n, 2) and not np.isnan(pos).any()
        for leaf in (64, 16):
            _check(nb, orc, pos, w, leaf, (name, n, leaf))


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_value_scenes_hold_what_their_names_say(dtype):
    n = 6000
    f64 = dtype == np.float64
    assert np.isneginf(S.special("neg_inf", dtype, n)[0]).sum() == 2
    p = S.special("pos_inf_x", dtype, n)[0]
    assert np.isposinf(p).sum() == 1 and np.isposinf(p[n // 2, 0])
    p = S.special("overflowing_sum", dtype, n)[0]
    with np.errstate(over="ignore"):
        assert np.isfinite(p).all() and np.isposinf(p[n // 2, 0] + p[n // 2 + 1, 0])
    p = S.special("overflowing_neg_sum", dtype, n)[0]
    with np.errstate(over="ignore"):
        assert np.isfinite(p).all() and np.isneginf(p[n // 2, 1] + p[n // 2 + 1, 1])
    p = S.special("subnormal_zero", dtype, n)[0]
    tiny = np.finfo(dtype).tiny
    assert ((p[::97, 0] > 0) & (p[::97, 0] < tiny)).all()                      # subnormal, not flushed
    assert (p[5::97, 1] == 0).all() and not np.signbit(p[5::97, 1]).any() and np.signbit(p[7::97, 1]).all()
    p = S.special("signed_wide", dtype, n)[0]
    assert (p < 0).any() and (p > 0).any() and np.abs(p).max() / np.abs(p).min() > 1e22
    p = S.special("cancel_pairs", dtype, n)[0]
    assert np.array_equal(p[1::2], -p[0::2])
    s = dtype(0)
    for x in p[:200, 0]:
        s = dtype(s + x)
    assert s == 0 and (1.7e308 if f64 else 3e38) > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_groups_put_the_roots_children_on_the_thresholds(nb, orc, dtype):
    for a, b in S.pairs(dtype):
        pos, w = S.two_groups(dtype, a, b)
        assert pos.shape[0] == a + b
        o = _check(nb, orc, pos, w, 64, (a, b))
        c0 = 1
        c1 = int(o.skip[c0])
        assert sorted((_points_below(o, c0), _points_below(o, c1))) == [a, b], (a, b)
        assert int(o.skip[c1]) == o.skip.shape[0]                          # the root has exactly these two children


def test_scenes_either_side_of_the_fused_partition_limit(nb, orc):
    for n in S.FUSED_EDGE:
        pos, w = S.uniform(np.float32, n)
        assert pos.shape[0] == n
        _check(nb, orc, pos, w, 64, n)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("base", S.ORDER_BASES)
def test_row_orders(nb, orc, dtype, base):
    pos, w = S.order_base(base, dtype)
    x = pos[:, 0]
    for leaf in (64, 8):
        def ids(p_, w_, leaf=leaf):
            return orc.BVH(p_, w_, leaf_size=leaf).flat().ids
        for order in S.ORDER_NAMES:
            p, ww = S.reorder(order, pos, w, ids)
            o = _check(nb, orc, p, ww, leaf, (base, order, leaf))
            if order == "ascending_x":
                assert (np.diff(p[:, 0]) >= 0).all()
            if order == "descending_x":
                assert (np.diff(p[:, 0]) <= 0).all()
            if order == "tree_order":   # nothing misplaced at any level: the two-pointer partition swaps nothing
                assert np.array_equal(o.ids, np.arange(p.shape[0])), (base, leaf)
            if order == "tree_order_reversed":
                assert np.array_equal(p, S.reorder("tree_order", pos, w, ids)[0][::-1])
    assert x.shape[0] in (20000, 6000)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cluster_scene_needs_more_node_ids_than_the_builders_reserve(nb, orc, dtype):
    leaf = 16
    pos, w = S.clusters(dtype, 64, leaf)
    n = pos.shape[0]
    assert n == 64 * 64 * (leaf + 2) == 73728
    # bvh_build_layout (bvh_build.hip) and bvh64_layout (bvh_build64.hip): node_cap = min(4 n / leaf, 2 n) + 4096
    reserve = min(4 * n // leaf, 2 * n) + 4096
    assert reserve == S.node_reserve(n, leaf) == 22528
    o = _check(nb, orc, pos, w, leaf, "clusters64")
    assert o.skip.shape[0] >= reserve + 2000, o.skip.shape[0]
    pos, w = S.clusters(dtype, 56, leaf)
    n = pos.shape[0]
    reserve = min(4 * n // leaf, 2 * n) + 4096
    assert reserve == 18208
    o = _check(nb, orc, pos, w, leaf, "clusters56")
    assert o.skip.shape[0] < reserve, o.skip.shape[0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_cluster_scene_keeps_its_node_count_over_the_steps_the_gpu_test_takes(orc, dtype):
    leaf = 16
    pos, w = S.clusters(dtype, 64, leaf)
    p, v, ww, ids, _ = orc.update_bvh(pos, np.zeros_like(pos), w, delta=1e-3, theta=1.0, leaf_size=leaf, nsteps=4, nthreads=16)
    # the rows as the fourth step's build sees them: three steps on
    p3, _, w3, _, _ = orc.update_bvh(pos, np.zeros_like(pos), w, delta=1e-3, theta=1.0, leaf_size=leaf, nsteps=3, nthreads=16)
    for rows, wts in ((p3, w3), (p, ww)):
        o = orc.BVH(rows, wts, leaf_size=leaf).flat()
        assert not o.overflow and o.skip.shape[0] >= S.node_reserve(rows.shape[0], leaf) + 2000, o.skip.shape[0]
