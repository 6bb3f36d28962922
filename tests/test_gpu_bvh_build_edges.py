"""The device BVH builders (f32: bvh_build.hip with bvh_fold / bvh_partition / bvh_subtrees / bvh_finish.hip; f64:
bvh_build64.hip) at their edges, against the CPU oracle, bit for bit.  Needs an MI355X.

  1  special values in the device chain: infinities, sums that overflow, subnormals and signed zeros, 24 signed decades,
     sums that return to exactly zero;
  2  nodes whose sizes sit exactly on a build-time threshold (kSub, kChunk, the use_runs rule, kRunLen, kFusedPartitionMax;
     kSmallNode, kSeg, kLongNode);
  3  rows that every partition finds in place already, and rows in the opposite order;
  4  a tree with more nodes than the builders reserve ids for: the build declines half-way, every later kernel still runs;
  5  the same inside a multi-step call, where the f32 verdict is taken on the device (bvh_step_ahead);
  6  a NaN that appears during a call.

The scenes come from tests/_bvh_edge_scenes.py; test_bvh_edge_scenes_host.py checks, without a GPU, that they are what is
assumed here.  No scene is skipped: the oracle overflows on none of them, and that is asserted."""
import numpy as np
import pytest

from tests import _bvh_edge_scenes as S

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
KEYS = ("mass", "is_leaf", "first", "count", "skip")


@pytest.fixture(scope="module")
def ctx(nb):
    c = nb._capi.Context(0)
    yield c
    c.close()


def _oracle_tree(orc, pos, w, leaf, tag):
    bvh = orc.BVH(pos, w, leaf_size=leaf)
    o = bvh.flat()
    assert not o.overflow, tag
    return bvh, o


def _tree_equal(t, o, tag):
    for k in KEYS:
        assert np.array_equal(t[k], getattr(o, k)), (tag, k)
    assert np.array_equal(t["geom"], o.geom, equal_nan=True), tag
    assert np.array_equal(t["order"], o.ids), tag


def _rows_equal(c, o, w, tag):
    p, _, w2, ids = c.download()
    assert np.array_equal(ids, o.ids), tag
    assert np.array_equal(p, o.pos_perm, equal_nan=True), tag
    assert np.array_equal(w2, w[o.ids]), tag


def _build_and_compare(C, c, orc, pos, w, leaf, tag, on_device=True, rows=True, theta=50.0, walk=False):
    """upload, one build by accel_tree, and the tree (and rows) against the oracle's.  walk: every row is a target."""
    bvh, o = _oracle_tree(orc, pos, w, leaf, tag)
    c.set_params(theta=theta, leaf_size=leaf)
    c.upload(pos, np.zeros_like(pos), w)
    acc = c.accel_tree(C.TREE_BVH, pos if walk else pos[:4])
    assert c.last_build_on_device() == on_device, tag
    _tree_equal(c.tree_export(), o, tag)
    if rows:
        _rows_equal(c, o, w, tag)
    if walk:
        ref = bvh.walk(pos, theta=theta, nthreads=16)
        assert np.array_equal(acc, ref, equal_nan=True), tag
    return o


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("leaf", [64, 16])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", S.SPECIAL_NAMES)
def test_special_values_build_on_the_device(nb, orc, ctx, name, dtype, leaf):
    """bvh_init / b64_init flag NaN only, so the device folds (bvh_big_fold, the prepared chunk runs, the in-LDS chain of
    bvh_subtrees; b64_fold, b64_fold_small) must carry infinities, overflowing sums, subnormals and exact cancellation as the
    sequential chain does.  At 6000 bodies the walk (theta 0.7) also meets the infinite boxes and centres of gravity."""
    C = nb._capi
    for n in S.SPECIAL_SIZES:
        pos, w = S.special(name, dtype, n)
        assert not np.isnan(pos).any()
        if n == 6000:
            _build_and_compare(C, ctx, orc, pos, w, leaf, (name, n), theta=0.7, walk=True)
        else:
            _build_and_compare(C, ctx, orc, pos, w, leaf, (name, n))


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("dtype,a,b", [(np.float32, a, b) for a, b in S.PAIRS_F32] + [(np.float64, a, b) for a, b in S.PAIRS_F64])
def test_children_exactly_on_the_size_thresholds(nb, orc, ctx, dtype, a, b):
    """The root's children hold exactly a and b points: either side of every `>` / `<=` on a node's length."""
    pos, w = S.two_groups(dtype, a, b)
    _build_and_compare(nb._capi, ctx, orc, pos, w, 64, (a, b))


@pytest.mark.parametrize("n", S.FUSED_EDGE)
def test_either_side_of_the_fused_partition_limit(nb, orc, ctx, n):
    """400 000 points: bvh_big_ranks swaps in the rank pass; 400 001: rank lists, then bvh_big_swap."""
    pos, w = S.uniform(np.float32, n)
    _build_and_compare(nb._capi, ctx, orc, pos, w, 64, n, rows=False)


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("leaf", [64, 8])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("base", S.ORDER_BASES)
def test_row_orders(nb, orc, ctx, base, dtype, leaf):
    """Nothing misplaced at any level (the rank lists are empty, no pair slot is ever posted), and the most misplaced."""
    pos, w = S.order_base(base, dtype)

    def ids(p_, w_):
        return orc.BVH(p_, w_, leaf_size=leaf).flat().ids
    for order in S.ORDER_NAMES:
        p, ww = S.reorder(order, pos, w, ids)
        o = _build_and_compare(nb._capi, ctx, orc, p, ww, leaf, (base, order))
        if order == "tree_order":
            assert np.array_equal(o.ids, np.arange(p.shape[0]))


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("dtype", DTYPES)
def test_out_of_node_ids_in_one_build(nb, orc, dtype):
    """24 575 nodes against 22 528 reserved ids (bvh_build_layout, bvh64_layout): the allocator raises the fallback flag
    half-way and every later kernel of the build runs on a half-made tree; the host builder then builds from rows that must be
    intact.  The next build in the same context fits and finds no flag or counter left behind."""
    C = nb._capi
    leaf = 16
    with C.Context(0) as c:
        pos, w = S.clusters(dtype, 64, leaf)
        o = _build_and_compare(C, c, orc, pos, w, leaf, "clusters64", on_device=False)
        assert o.skip.shape[0] > S.node_reserve(pos.shape[0], leaf)
        pos, w = S.clusters(dtype, 56, leaf)
        o = _build_and_compare(C, c, orc, pos, w, leaf, "clusters56", on_device=True)
        assert o.skip.shape[0] < S.node_reserve(pos.shape[0], leaf)


# ------------------------------------------------------------------ 5, 6
def _verdict_lines(err, capfd):
    """(verdict, nodes, fallback) of every 'step ahead: build verdict' line of the trace (shown before anything is asserted)."""
    out = []
    for ln in err.splitlines():
        if "step ahead: build verdict" not in ln:
            continue
        with capfd.disabled():
            print(ln)
        tail = ln.split("build verdict")[1]
        out.append((int(tail.split()[0]), int(tail.split("(")[1].split()[0]), int(tail.split("fallback")[1].split()[0].rstrip(","))))
    return out


def _steps_equal(c, orc, pos, vel, w, delta, theta, leaf, nsteps, tag):
    p, v, w2, ids = c.download()
    rp, rv, rw, rids, _ = orc.update_bvh(pos, vel, w, delta=delta, theta=theta, leaf_size=leaf, mode=orc.AS_WRITTEN, nsteps=nsteps,
                                         nthreads=16)
    assert np.array_equal(ids, rids), tag
    assert np.array_equal(p, rp, equal_nan=True) and np.array_equal(v, rv, equal_nan=True), tag
    assert np.array_equal(w2, rw), tag


def test_out_of_node_ids_over_steps_f32(nb, orc, monkeypatch, capfd):
    """The same scene over four steps of one call.  The first step takes the plain sequence (no walk to estimate from yet); from
    the second on the step is enqueued ahead: the device concludes 'verdict 0' with the fallback flag up, the walk returns at
    once, the integration is never enqueued, and the plain sequence (device build declined again, host builder) does the step
    from the rows the step started with."""
    C = nb._capi
    leaf, delta, theta = 16, 1e-3, 1.0
    pos, w = S.clusters(np.float32, 64, leaf)
    vel = np.zeros_like(pos)
    monkeypatch.setenv("NBODY_TRACE", "1")
    with C.Context(0) as c:
        c.set_params(theta=theta, leaf_size=leaf)
        c.upload(pos, vel, w)
        c.update_tree(C.TREE_BVH, delta, 4)
        assert not c.last_build_on_device()
        _steps_equal(c, orc, pos, vel, w, delta, theta, leaf, 4, "clusters64")
    lines = _verdict_lines(capfd.readouterr().err, capfd)
    assert any(v == 0 and fb == 1 for v, _, fb in lines), lines
    assert not any(v == 1 for v, _, _ in lines), lines


def test_out_of_node_ids_over_steps_f64(nb, orc):
    C = nb._capi
    leaf, delta, theta = 16, 1e-3, 1.0
    pos, w = S.clusters(np.float64, 64, leaf)
    vel = np.zeros_like(pos)
    with C.Context(0) as c:
        c.set_params(theta=theta, leaf_size=leaf)
        c.upload(pos, vel, w)
        c.update_tree(C.TREE_BVH, delta, 4)
        assert not c.last_build_on_device()
        _steps_equal(c, orc, pos, vel, w, delta, theta, leaf, 4, "clusters64")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_that_appears_during_the_call(nb, orc, monkeypatch, capfd, dtype):
    """One velocity is NaN: the first step builds on the device, and moves that body to a NaN position; every later build
    declines (bvh_init / b64_init) — at f32 on the step enqueued ahead, whose verdict the device takes.  The rows the plain
    sequence then starts from must be the ones the step started with.  theta is the library's default, 50: nearly every node
    is accepted and a target meets few terms (at theta 0.7 a walk over 8192 uniform bodies takes more than n / 16 terms per
    target, the driver switches to the fused walk, walk_near_direct, and no step is enqueued ahead).  The same bodies with a
    finite velocity, in the same context, then step on the device as if nothing had happened."""
    C = nb._capi
    n, leaf, delta, theta = 8192, 64, 0.1, 50.0
    rng = np.random.default_rng(6000)
    pos = (rng.random((n, 2)) * 1e5).astype(dtype)
    vel = rng.standard_normal((n, 2)).astype(dtype)
    w = S.weights(n)
    bad = vel.copy()
    bad[4000, 0] = np.nan
    f32 = dtype == np.float32
    monkeypatch.setenv("NBODY_TRACE", "1")
    with C.Context(0) as c:
        c.set_params(theta=theta, leaf_size=leaf)
        c.upload(pos, bad, w)
        c.update_tree(C.TREE_BVH, delta, 5)
        assert not c.last_build_on_device()
        _steps_equal(c, orc, pos, bad, w, delta, theta, leaf, 5, "nan")
        err = capfd.readouterr().err
        lines = _verdict_lines(err, capfd)
        # step 1 (every position finite still) built on the device, the four after it on the host
        built = [ln for ln in err.splitlines() if ("device bvh build:" in ln if f32 else "device bvh build (f64)" in ln and "fallback 0" in ln)]
        hosted = [ln for ln in err.splitlines() if "host tree build:" in ln]
        with capfd.disabled():
            print("\n".join(built + hosted))
        assert len(built) == 1 and len(hosted) == 4, err[-2000:]
        if f32:
            assert any(v == 0 and fb == 1 for v, _, fb in lines), lines
            assert not any(v == 1 for v, _, _ in lines), lines
        c.upload(pos, vel, w)
        c.update_tree(C.TREE_BVH, delta, 3)
        assert c.last_build_on_device()
        _steps_equal(c, orc, pos, vel, w, delta, theta, leaf, 3, "finite")
        lines = _verdict_lines(capfd.readouterr().err, capfd)
        if f32:
            assert len(lines) >= 2 and all(v == 1 for v, _, _ in lines[-2:]), lines
