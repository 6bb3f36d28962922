"""The device quad-tree build (quad_build.hip, quad_build_device in tree_build_driver.hip) at its edges, against the CPU
oracle, bit for bit and with signed zeros told apart.  Needs an MI355X.

  1  the 31 child codes of the path key: a leaf at depth 31 builds on the device, one at depth 32 is declined;
  2  the sort depth (the last tree's depth plus 3, at most 31) and the re-sort when the tree turns out deeper;
  3  the 17-key window of qb_leaf_order at the ends of the sorted keys, across a work-group's edge, over two full leaves;
  4  points exactly on cell midlines (the strict `>` of qb_path_keys);
  5  NaN, infinite, signed-zero, subnormal and huge positions;
  6  u32 masses that wrap, node masses of exactly 0, bodies without weight;
  7  other root cells: centred, at (-0.0, -0.0), far smaller than the cloud;
  8  a tree that gets twenty levels deeper, and one deeper than the key, inside one multi-step call.

The scenes come from tests/_quad_edge_scenes.py; test_quad_edge_scenes_host.py checks, without a GPU, that they are what is
assumed here.  No scene is skipped: the oracle overflows on none but nan_nine, which must be an error."""
import numpy as np
import pytest

from tests import _quad_edge_scenes as S

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]
TRACE = "device quad build: sorted by"


@pytest.fixture(scope="module")
def ctx(nb):
    c = nb._capi.Context(0)
    yield c
    c.close()


def _oracle(orc, pos, w, root, tag):
    q = orc.Quad(pos, w, root=root)
    o = q.flat()
    assert not o.overflow, tag
    return q, o


def _tree_check(c, o, on_device, tag):
    """The three things every build is held to: where it was built, its depth, and the tree bit for bit."""
    t = c.tree_export()
    assert c.last_build_on_device() == on_device, (tag, "built on the device" if on_device else "declined")
    assert t["max_depth"] == int(o.depth.max()), (tag, t["max_depth"], int(o.depth.max()))
    S.tree_equal_bits(t, o, tag)


def _build_and_compare(C, c, orc, pos, w, tag, root=S.ROOT, on_device=True, theta=0.5, walk=False):
    """upload, one build by accel_tree, the tree against the oracle's.  walk: every row is a target, against the oracle's walk."""
    q, o = _oracle(orc, pos, w, root, tag)
    c.set_params(theta=theta, quad_root_x=root[0], quad_root_y=root[1], quad_root_h=root[2])
    c.upload(pos, np.zeros_like(pos), w)
    acc = c.accel_tree(C.TREE_QUAD, pos if walk else pos[:4])
    _tree_check(c, o, on_device, tag)
    if walk:
        ref = q.walk(pos, theta=theta, nthreads=16)
        assert np.array_equal(acc, ref, equal_nan=True), (tag, "walk")
    p, _, w2, ids = c.download()                       # the quad build keeps the rows where they are
    assert np.array_equal(ids, np.arange(pos.shape[0])) and np.array_equal(w2, w), tag
    assert np.array_equal(p.view(np.uint8), pos.view(np.uint8)), tag
    return o


def _trace_lines(err, capfd):
    """[(levels, flags, nodes, depth)] of every 'device quad build' line of the trace (shown before anything is asserted)."""
    out = []
    for ln in err.splitlines():
        if TRACE not in ln:
            continue
        with capfd.disabled():
            print(ln)
        tail = ln.split(TRACE)[1].replace(",", " ").split()    # <L> levels flags <F> <M> nodes depth <D>
        out.append((int(tail[0]), int(tail[3]), int(tail[4]), int(tail[7])))
    return out


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("corner", ["sw"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_key_limit_31_levels_on_the_device_32_declined(nb, orc, ctx, dtype, corner):
    """`ld > kLevels` in qb_leaf_order from both sides, and every shift `2 * (kLevels - ld)` at ld == 31 (0 bits): a leaf of 31
    child codes fills the key and builds on the device; one of 32 is beyond it and goes to the host builder, which must find
    the rows intact.  The declined build leaves nothing behind: a shallow scene is a device build again."""
    C = nb._capi
    for D, on_device in ((30, True), (31, True), (32, False), (33, False), (31, True), (32, False)):
        pos, w, _ = S.exact(dtype, D, 300, corner)
        o = _build_and_compare(C, ctx, orc, pos, w, (corner, D), on_device=on_device)
        assert int(o.depth.max()) == D
        pos, w, _ = S.exact(dtype, 8, 300, corner)
        _build_and_compare(C, ctx, orc, pos, w, (corner, D, "then 8"), on_device=True)


# ------------------------------------------------------------------ 2
SORT_SEQUENCE = ((10, 1), (13, 1), (17, 2), (12, 1), (29, 2), (31, 1))


class _DeviceCopy:
    """A numpy array's bytes in device memory, for the device-pointer calls: allocated and filled through the HIP runtime the
    library itself is linked against (its symbols resolve through the library's handle).  hipMemcpy returns when the copy is done."""

    def __init__(self, lib, a):
        import ctypes
        self.free = lib.hipFree
        self.free.restype, self.free.argtypes = ctypes.c_int, [ctypes.c_void_p]
        malloc, memcpy = lib.hipMalloc, lib.hipMemcpy
        malloc.restype, malloc.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        memcpy.restype, memcpy.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        a = np.ascontiguousarray(a)
        p = ctypes.c_void_p()
        assert malloc(ctypes.byref(p), a.nbytes) == 0 and p.value
        self.ptr = p.value
        assert memcpy(self.ptr, a.ctypes.data, a.nbytes, 1) == 0        # hipMemcpyHostToDevice

    def close(self):
        if self.ptr:
            assert self.free(self.ptr) == 0
            self.ptr = None


@pytest.mark.parametrize("dtype", DTYPES)
def test_sort_depth_and_the_redo(nb, orc, monkeypatch, capfd, dtype):
    """quad_build_device sorts by the last tree's depth plus 3 (31 on a fresh upload, and never more than 31): a tree exactly
    3 levels deeper builds in one pass, one 4 levels deeper raises flag 2 and is sorted again by all 31.  An upload forgets the
    last depth, so after the first scene the rows are replaced in place (nbody_import_rows_dev) and the context keeps it.
    Depths 10, 13, 17, 12, 29, 31: sorted by 31; 13; 16 then 31; 20; 15 then 31; 31 (29 + 3 clamped)."""
    C = nb._capi
    n = 300
    monkeypatch.setenv("NBODY_TRACE", "1")
    seen = []
    with C.Context(0) as c:
        c.set_params(theta=0.5)
        for k, (D, _) in enumerate(SORT_SEQUENCE):
            pos, w, _ = S.exact(dtype, D, n, "sw")
            q, o = _oracle(orc, pos, w, S.ROOT, D)
            assert int(o.depth.max()) == D
            if k == 0:
                c.upload(pos, np.zeros_like(pos), w)
            else:
                assert np.array_equal(w, S.weights(n))                 # the weights stay: only positions are replaced
                bufs = [_DeviceCopy(c.lib, a) for a in (np.arange(n, dtype=np.uint32), pos, np.zeros_like(pos))]
                try:
                    c.import_rows_dev(n, *(b.ptr for b in bufs))       # (returns when the rows are in place)
                finally:
                    for b in bufs:
                        b.close()
            capfd.readouterr()
            acc = c.accel_tree(C.TREE_QUAD, pos)
            lines = _trace_lines(capfd.readouterr().err, capfd)
            seen.append((D, lines))
            _tree_check(c, o, True, D)
            assert np.array_equal(acc, q.walk(pos, theta=0.5, nthreads=16)), D
            assert np.array_equal(c.download()[0], pos), D
    expect_first = (31, 13, 16, 20, 15, 31)
    for (D, count), first, (_, lines) in zip(SORT_SEQUENCE, expect_first, seen):
        assert len(lines) == count, (D, lines)
        assert lines[0][0] == first, (D, lines)
        assert lines[-1][1] == 0 and lines[-1][3] == D, (D, lines)     # the pass that stands: no flag, the oracle's depth
        if count == 2:
            assert lines[0][1] & 2, (D, lines)                        # "deeper than sorted"
            assert lines[1][0] == 31, (D, lines)


# ------------------------------------------------------------------ 3
@pytest.mark.parametrize("corner,D", [("sw", 12), ("ne", 12), ("ne", 20)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_window_at_the_ends_of_the_sorted_keys(nb, orc, ctx, dtype, corner, D):
    """The nine rows that set the depth are the first (sw) or the last (ne) of the sorted keys: their windows keys[r-8 .. r+8]
    run off the array (s < 0, s + 8 >= n).  n = 9: nothing else; 255, 256, 257: the last nine end before, at and across the
    edge of a 256-thread group, whose other threads are bystanders."""
    C = nb._capi
    for n in (9, 16, 17, 255, 256, 257):
        pos, w, rows = S.exact(dtype, D, n, corner)
        o = _build_and_compare(C, ctx, orc, pos, w, (corner, D, n), walk=True)
        got = o.order[:9] if corner == "sw" else o.order[-9:]
        assert sorted(got.tolist()) == rows.tolist()


@pytest.mark.parametrize("D", [6, 12])
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_full_leaves_side_by_side(nb, orc, ctx, dtype, D):
    """Sixteen consecutive keys, eight per leaf: a window of nine always reaches into the sibling, the run of a leaf's own keys
    is seven places each way and must stop at the sibling's, and the rank by index orders rows that the sort left scattered."""
    pos, w, ra, rb = S.siblings_full(dtype, D)
    o = _build_and_compare(nb._capi, ctx, orc, pos, w, ("siblings", D), walk=True)
    a = int(np.flatnonzero((o.is_leaf != 0) & (o.count == 8) & (o.depth == D))[0])
    assert o.order[o.first[a]:o.first[a] + 16].tolist() == ra.tolist() + rb.tolist()


@pytest.mark.parametrize("dtype", DTYPES)
def test_root_is_a_leaf(nb, orc, ctx, dtype):
    for n in (1, 8):
        pos, w = S.uniform(dtype, n)
        o = _build_and_compare(nb._capi, ctx, orc, pos, w, n, walk=True)
        assert o.skip.shape[0] == 1


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("root", S.LATTICE_ROOTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_points_on_midlines(nb, orc, ctx, dtype, root):
    """Every coordinate is a cell border: `>` sends the point to the low side, `>=` would send it to the high side (the host
    test shows the oracle builds another tree one ulp up)."""
    pos, w = S.midline_lattice(dtype, root)
    _build_and_compare(nb._capi, ctx, orc, pos, w, root, root=root, theta=0.5, walk=True)


# ------------------------------------------------------------------ 5
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [s for s in S.SPECIAL_NAMES if s != "nan_nine"])
def test_special_values_build_on_the_device(nb, orc, ctx, name, dtype):
    """The device build flags nothing: a NaN takes child 0 at every level, an infinity the far edge, and the sums and
    quotients of the upward pass must overflow and cancel as the sequential ones do."""
    pos, w = S.special(name, dtype)
    _build_and_compare(nb._capi, ctx, orc, pos, w, name, theta=0.7, walk=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nine_nan_rows_are_an_error_and_leave_nothing_behind(nb, orc, ctx, dtype):
    C = nb._capi
    pos, w = S.special("nan_nine", dtype)
    ctx.set_params(theta=0.7, quad_root_x=S.ROOT[0], quad_root_y=S.ROOT[1], quad_root_h=S.ROOT[2])
    ctx.upload(pos, np.zeros_like(pos), w)
    with pytest.raises(C.NBodyError) as e:
        ctx.accel_tree(C.TREE_QUAD, pos[:4])
    assert e.value.code == C.ERR_DEGENERATE
    assert not ctx.last_build_on_device()
    pos, w = S.special("zeros_subnormals", dtype)
    _build_and_compare(C, ctx, orc, pos, w, "after nan_nine", theta=0.7, walk=True)


# ------------------------------------------------------------------ 6
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scene", ["uniform", "lattice"])
@pytest.mark.parametrize("name", S.MASS_NAMES)
def test_wrapping_masses(nb, orc, ctx, name, scene, dtype):
    """u32 sums that wrap (qb_leaf_stats, qb_internal_stats), nodes whose mass is exactly 0 (bx / 0: infinite or NaN), and
    the conversion of masses up to 2^32 - 1 to the tree's precision."""
    pos = S.uniform(dtype, 500)[0] if scene == "uniform" else S.midline_lattice(dtype)[0]
    w = S.masses(name, pos.shape[0])
    o = _build_and_compare(nb._capi, ctx, orc, pos, w, (name, scene), theta=0.5, walk=True)
    if name != "full_range":
        assert ((o.is_leaf == 0) & (o.mass == 0)).any()


# ------------------------------------------------------------------ 7
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", S.ROOT_NAMES)
def test_other_root_cells(nb, orc, ctx, name, dtype):
    """neg_zero: child 0 takes its parent's offset as it is, so -0.0 survives down the chain of first children, while every
    other child's `offset + 0.0` is +0.0 (quad_tree.rs:183-186); tree_equal_bits tells them apart."""
    pos, w, root = S.roots(name, dtype)
    o = _build_and_compare(nb._capi, ctx, orc, pos, w, name, root=root, theta=0.5, walk=True)
    if name == "neg_zero":
        assert np.signbit(o.geom[:, :2]).sum() >= 6


# ------------------------------------------------------------------ 8
def _builds(err, capfd):
    """The builds of a call in order: ("device", levels, flags, depth) per pass of the device build, ("host",) per host build."""
    out = []
    for ln in err.splitlines():
        if TRACE in ln:
            tail = ln.split(TRACE)[1].replace(",", " ").split()
            out.append(("device", int(tail[0]), int(tail[3]), int(tail[7])))
        elif "host tree build:" in ln:
            out.append(("host",))
        else:
            continue
        with capfd.disabled():
            print(ln)
    return out


def _steps_equal(c, orc, pos, vel, w, nsteps, tag):
    p, v, w2, ids = c.download()
    rp, rv, _ = orc.update_quad(pos, vel, w, delta=S.COLLAPSE_DELTA, theta=0.5, nsteps=nsteps, nthreads=16)
    assert np.array_equal(ids, np.arange(pos.shape[0])) and np.array_equal(w2, w), tag
    assert np.array_equal(p.view(np.uint8), rp.view(np.uint8)), (tag, "positions")
    assert np.array_equal(v.view(np.uint8), rv.view(np.uint8)), (tag, "velocities")


@pytest.mark.parametrize("dtype", DTYPES)
def test_redo_inside_one_call(nb, orc, monkeypatch, capfd, dtype):
    """Depths 5, 25, 5 over the three builds of one update_tree call: the second sorts by 8 levels, finds flag 2 and sorts
    again by 31; the third sorts by 28."""
    C = nb._capi
    pos, vel, w, _ = S.collapse(dtype)
    monkeypatch.setenv("NBODY_TRACE", "1")
    with C.Context(0) as c:
        c.set_params(theta=0.5)
        c.upload(pos, vel, w)
        capfd.readouterr()
        c.update_tree(C.TREE_QUAD, S.COLLAPSE_DELTA, 3)
        b = _builds(capfd.readouterr().err, capfd)
        assert c.last_build_on_device()
        _steps_equal(c, orc, pos, vel, w, 3, "collapse")
    assert [x[0] for x in b] == ["device"] * 4, b
    assert [(x[1], x[3]) for x in b] == [(31, 5), (8, b[1][3]), (31, 25), (28, 5)], b
    assert b[1][2] & 2 and not b[0][2] and not b[2][2] and not b[3][2], b


def test_too_deep_inside_one_call(nb, orc, monkeypatch, capfd):
    """f64: the second build of the call is deeper than the key: sorted by 7, again by 31, declined (flag 1), built on the
    host; the third is a device build again, sorted by all 31 levels as after any declined build."""
    C = nb._capi
    pos, vel, w, _ = S.collapse_deep()
    monkeypatch.setenv("NBODY_TRACE", "1")
    with C.Context(0) as c:
        c.set_params(theta=0.5)
        c.upload(pos, vel, w)
        capfd.readouterr()
        c.update_tree(C.TREE_QUAD, S.COLLAPSE_DELTA, 3)
        b = _builds(capfd.readouterr().err, capfd)
        assert c.last_build_on_device()
        _steps_equal(c, orc, pos, vel, w, 3, "collapse_deep")
    assert [x[0] for x in b] == ["device", "device", "device", "host", "device"], b
    assert b[0][1] == 31 and not b[0][2] and b[1][1] == b[0][3] + 3 and b[1][2] & 2, b
    assert b[2][1] == 31 and b[2][2] & 1, b
    assert b[4][1] == 31 and not b[4][2] and b[4][3] <= 10, b
