"""Frames of an ensemble on the device (frames() of the eight ensemble classes over nbody_frames_*): every world's tile against the
oracle's draw() of that world's own rows — its bodies, then its tracers as rows of weight 1 — with np.array_equal: byte
equality, no tolerance.  The scene is tests/_frames_scene.py (seven worlds that share their positions and differ in their
velocities and weights, with the planted rows its docstring lists); test_ensemble_frames_host.py checks on the CPU that the
oracle treats each planted row as the scene says.  Needs an MI355X.

Shapes.  Uniform classes: n in {1, 256, 257, 600} (the block's stride over rows is 256), the restricted ones with m in {0, 300}.
Ragged classes: sizes [1, 2, 257, 64, 600, 4096, 255], the ragged restricted ones with tracer counts [0, 1, 300, 0, 257, 1000, 5].
render_px 100 (the largest that fits the LDS route), 8 and 1 take the LDS route, 125 the global one."""
import numpy as np
import pytest

import _frames_scene as S

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
W = 7
H = 100_000
DT = 0.1
RAGGED_N = [1, 2, 257, 64, 600, 4096, 255]
RR_M = [0, 1, 300, 0, 257, 1000, 5]

# (class name, dtype, ragged, has tracers, the handle's word in its messages)
KINDS = {
    "ensemble": ("Ensemble", F32, False, False, "ensemble"),
    "ensemble64": ("Ensemble64", F64, False, False, "ensemble"),
    "ragged": ("RaggedEnsemble", F32, True, False, "ragged"),
    "ragged64": ("RaggedEnsemble64", F64, True, False, "ragged"),
    "restricted": ("RestrictedEnsemble", F32, False, True, "restricted"),
    "restricted64": ("RestrictedEnsemble64", F64, False, True, "restricted"),
    "rr": ("RaggedRestrictedEnsemble", F32, True, True, "ragged restricted"),
    "rr64": ("RaggedRestrictedEnsemble64", F64, True, True, "ragged restricted"),
}


def _shapes():
    out = []
    for kind, (_, _, ragged, tracers, _) in KINDS.items():
        if ragged:
            out.append((kind, tuple(RAGGED_N), tuple(RR_M) if tracers else (0,) * W))
        else:
            for n in (1, 256, 257, 600):
                for m in ((0, 300) if tracers else (0,)):
                    out.append((kind, (n,) * W, (m,) * W))
    return out


SHAPES = _shapes()
# one shape per class for the cases that build further handles: the uniform ones at n = 257 (and m = 300)
ONE_EACH = [s for s in SHAPES if KINDS[s[0]][2] or (s[1][0] == 257 and s[2][0] == (300 if KINDS[s[0]][3] else 0))]


def _id(shape):
    kind, sizes, counts = shape
    return kind if KINDS[kind][2] else f"{kind}-n{sizes[0]}-m{counts[0]}"


class Case:
    """A shape's scene and how to put (some of) its worlds on the device."""

    def __init__(self, nb, shape, height=H):
        self.nb, (self.kind, self.sizes, self.counts), self.height = nb, shape, height
        self.cls_name, self.dtype, self.ragged, self.has_tracers, self.who = KINDS[self.kind]
        self.worlds = S.scene(self.sizes, self.counts, self.dtype, height)
        self._expected = {}

    def make(self, which=None, tracers=True):
        """The class's ensemble of the worlds `which` (default: all); tracers=False: uploaded without its tracers."""
        ws = self.worlds if which is None else [self.worlds[k] for k in which]
        cls = getattr(self.nb, self.cls_name)
        pos, vel, w = [x["pos"] for x in ws], [x["vel"] for x in ws], [x["w"] for x in ws]
        if self.ragged:
            if not self.has_tracers:
                return cls(pos, vel, w)
            return cls(pos, vel, w, [(x["tpos"], x["tvel"]) if len(x["tpos"]) else None for x in ws] if tracers else None)
        pos, vel, w = np.stack(pos), np.stack(vel), np.stack(w)
        if not self.has_tracers:
            return cls(pos, vel, w)
        return cls(pos, vel, w, (np.stack([x["tpos"] for x in ws]), np.stack([x["tvel"] for x in ws])) if tracers else None)

    def frames(self, ens, render_px, tracers=False, height=None):
        height = self.height if height is None else height
        return ens.frames(height, render_px, tracers) if self.has_tracers else ens.frames(height, render_px)

    def state(self, ens):
        """-> per world (pos, vel, tpos, tvel) as the handle holds them now."""
        p, v, _ = ens.particles()
        n = len(self.sizes)
        empty = np.zeros((0, 2), self.dtype)
        if not self.has_tracers:
            return [(p[k], v[k], empty, empty) for k in range(n)]
        t = ens.tracers()
        if self.ragged:
            return [(p[k], v[k], t[k][0], t[k][1]) for k in range(n)]
        return [(p[k], v[k], t[0][k], t[1][k]) for k in range(n)]

    def expected(self, orc, render_px, tracers=False, state=None):
        """The oracle's draw() per world, stacked; of the scene as uploaded it is computed once and shared."""
        if state is not None:
            return np.stack([S.draw_world(orc, x, self.height, render_px, tracers, st) for x, st in zip(self.worlds, state)])
        key = (render_px, bool(tracers) and self.has_tracers)
        if key not in self._expected:
            e = np.stack([S.draw_world(orc, x, self.height, render_px, tracers) for x in self.worlds])
            e.setflags(write=False)
            self._expected[key] = e
        return self._expected[key]

    def tracer_flags(self):
        return (False, True) if self.has_tracers else (False,)


def _message(err):
    """The library's own message: NBodyError puts "nbody_hip error <code>: " in front of it."""
    head = f"nbody_hip error {err.code}: "
    assert str(err).startswith(head)
    return str(err)[len(head):]


def _same(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    for k in range(len(want)):
        assert np.array_equal(got[k], want[k]), f"{what}: world {k}: {int((got[k] != want[k]).any(axis=-1).sum())} pixels differ"


@pytest.fixture(scope="module", params=SHAPES, ids=_id)
def case(request, nb):
    c = Case(nb, request.param)
    c.ens = c.make()          # shared by the tests that only look; never stepped
    yield c
    c.ens.close()


@pytest.fixture(params=ONE_EACH, ids=_id)
def one(request, nb):
    """One shape per class, for the cases that put handles of their own on the device."""
    return Case(nb, request.param)


@pytest.fixture(params=[s for s in ONE_EACH if KINDS[s[0]][3]], ids=_id)
def one_with_tracers(request, nb):
    return Case(nb, request.param)


# ---- 1, 2: both routes against the oracle
@pytest.mark.parametrize("render_px", [100, 8, 1, 125])
def test_every_tile_is_the_oracles_draw_of_that_world(case, orc, render_px):
    for tracers in case.tracer_flags():
        got = case.frames(case.ens, render_px, tracers)
        assert got.shape == (W, render_px, render_px, 4)
        _same(got, case.expected(orc, render_px, tracers), f"render_px {render_px}, tracers {tracers}")
    if render_px == 100 and case.sizes[0] >= S.N_PLANTED and not case.ragged:
        # the planted pixels, seen on the device's own bytes (every world of a uniform shape has them)
        f = case.frames(case.ens, 100)
        assert (f[:, S.ROW, [10, 12, 14], 3] == [240, 250, 250]).all()
        assert (f[:, S.ROW, [20, 22, 31, 42]] == (0, 255, 0, 255)).all()
        assert (f[:, S.ROW, 35] == (255, 229, 229, 20)).all()


def test_the_two_routes_and_repeated_calls_agree(case, orc):
    """The same scene at render_px 100, 125, 100 again: the scratch of one route is not the other's, and growing it keeps nothing."""
    a = case.frames(case.ens, 100)
    case.frames(case.ens, 125)
    case.frames(case.ens, 250)       # the global route's buffers grow
    b = case.frames(case.ens, 100)
    assert np.array_equal(a, b)
    _same(case.frames(case.ens, 125), case.expected(orc, 125), "render_px 125 after 250")


# ---- 3: another cell size
def test_height_800_with_cells_of_8(one, orc, nb):
    c = Case(nb, (one.kind, one.sizes, one.counts), height=800)
    with c.make() as ens:
        for tracers in c.tracer_flags():
            _same(c.frames(ens, 100, tracers), c.expected(orc, 100, tracers), f"height 800, tracers {tracers}")
        _same(c.frames(ens, 200), c.expected(orc, 200), "height 800, cells of 4, the global route")


# ---- 4: independence
def test_a_tile_is_that_of_the_world_alone(one):
    tracers = one.has_tracers
    with one.make() as ens:
        whole = {px: one.frames(ens, px, tracers) for px in (100, 125)}
    for k in range(W):
        with one.make([k]) as alone:
            for px in (100, 125):
                f = one.frames(alone, px, tracers)
                assert f.shape == (1, px, px, 4) and np.array_equal(f[0], whole[px][k]), (k, px)


# ---- 5: the single-world path
@pytest.mark.parametrize("render_px", [100, 125])
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] in ("ensemble", "restricted")], ids=_id)
def test_f32_uniform_equals_the_single_world_render(shape, nb, render_px):
    case = Case(nb, shape)
    ctx = nb._capi.Context(0)
    try:
        with case.make() as ens:
            got_of = {tracers: case.frames(ens, render_px, tracers) for tracers in case.tracer_flags()}
        for tracers, got in got_of.items():
            for k, x in enumerate(case.worlds):
                ctx.upload(x["pos"], x["vel"], x["w"])
                if tracers and len(x["tpos"]):
                    ctx.upload_tracers(x["tpos"], x["tvel"])
                single = ctx.render(H, render_px, tracers=bool(tracers and len(x["tpos"])))
                assert np.array_equal(got[k], single), (k, tracers)
    finally:
        ctx.close()


# ---- 6: the current half of the double buffer
def test_frames_follow_the_steps(one, orc):
    with one.make() as ens:
        for step in (1, 2):
            ens.update(DT, None, n_steps=1)
            st = one.state(ens)
            for tracers in one.tracer_flags():
                for px in (100, 125):
                    _same(one.frames(ens, px, tracers), one.expected(orc, px, tracers, state=st), f"after step {step}, render_px {px}")


# ---- 7: the state is untouched
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _assert_states_equal(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        for u, v in zip(x, y):
            assert u.shape == v.shape and np.array_equal(_bits(u), _bits(v)), (what, k)


def test_frames_leave_the_state_alone(one):
    with one.make() as ens, one.make() as twin:
        before = one.state(ens)
        for px in (100, 125):
            one.frames(ens, px, one.has_tracers)
        _assert_states_equal(one.state(ens), before, "frames() moved a row")
        for step in range(3):
            one.frames(ens, 100 if step % 2 else 125, one.has_tracers)
            ens.update(DT, None, n_steps=1)
            twin.update(DT, None, n_steps=1)
        one.frames(ens, 100, one.has_tracers)
        _assert_states_equal(one.state(ens), one.state(twin), "frames between steps changed the steps")


# ---- 8: tracers asked of a handle that holds none
def test_tracers_without_tracers_are_the_bodies_frames(one_with_tracers, orc):
    one = one_with_tracers
    with one.make(tracers=False) as ens:
        for px in (100, 125):
            a, b = ens.frames(H, px, tracers=False), ens.frames(H, px, tracers=True)
            assert np.array_equal(a, b)
            _same(b, one.expected(orc, px, False), f"no tracers, render_px {px}")
        if one.ragged:
            return
        # and after tracers come and go again
        ens.set_tracers((np.stack([x["tpos"] for x in one.worlds]), np.stack([x["tvel"] for x in one.worlds])))
        _same(ens.frames(H, 100, tracers=True), one.expected(orc, 100, True), "tracers set")
        ens.set_tracers(None)
        _same(ens.frames(H, 100, tracers=True), one.expected(orc, 100, False), "tracers removed")


def test_rr_tracers_replaced_after_a_frame(nb, orc):
    """The ragged handles cache their table of row ranges: new counts must replace it."""
    c = Case(nb, ("rr", tuple(RAGGED_N), tuple(RR_M)))
    d = Case(nb, ("rr", tuple(RAGGED_N), tuple(reversed(RR_M))))
    with c.make() as ens:
        _same(ens.frames(H, 100, tracers=True), c.expected(orc, 100, True), "first counts")
        ens.set_tracers([(x["tpos"], x["tvel"]) if len(x["tpos"]) else None for x in d.worlds])
        for px in (100, 125):
            _same(ens.frames(H, px, tracers=True), d.expected(orc, px, True), f"second counts, render_px {px}")
        _same(ens.frames(H, 100, tracers=False), c.expected(orc, 100, False), "the bodies are the same")


# ---- 9: refusals
def test_refusals_name_frames_and_leave_the_handle_working(one, orc, nb):
    C = nb._capi
    with one.make() as tmp:
        handle_cls = type(tmp.h)
    empty = handle_cls(0)
    try:
        with pytest.raises(C.NBodyError) as e:
            empty.frames(H, 100)
        assert e.value.code == C.ERR_INVALID and _message(e.value).startswith(one.who + " frames") and "nothing uploaded" in str(e.value)
    finally:
        empty.close()
    with one.make() as ens:
        def refused(height, render_px, tracers=False, also=None):
            with pytest.raises(C.NBodyError) as e:
                one.frames(ens, render_px, tracers, height=height)
            msg = _message(e.value)
            assert e.value.code == C.ERR_INVALID and msg.startswith(one.who + " frames") and (also is None or also in msg), msg

        refused(0, 100)
        refused(H, 0)
        refused(H, 7)                      # 7 does not divide 100 000
        refused(100, 1000)                 # nor does a render_px above the height
        refused(1 << 25, 2)                # as nbody_render_rgba: height <= 2^24
        refused(H, 3125, also="2^26")      # 7 * 3125^2 = 6.8e7 pixels > 2^26, before anything is allocated
        # rgba_out NULL, through the C call
        fn = getattr(C.load(), "nbody_frames_" + ens.h._prefix[len("nbody_"):])
        args = (H, 100, 0) if one.has_tracers else (H, 100)
        assert fn(ens.h.h, *args, None) == C.ERR_INVALID
        msg = ens.h._call("_last_error").decode()
        assert msg.startswith(one.who + " frames") and "rgba_out" in msg
        for tracers in one.tracer_flags():
            _same(one.frames(ens, 100, tracers), one.expected(orc, 100, tracers), "after the refusals")


def test_more_than_2_24_rows_in_a_world_are_refused_with_tracers_only(nb, orc):
    """One world of one body and 2^24 tracers: n + m = 2^24 + 1 rows do not fit beside v in a word.  Without the tracers the
    world is painted; with one tracer fewer it is painted with them."""
    C = nb._capi
    m = 1 << 24
    pos, vel, w = np.array([[[10.5, 20.5]]], F32), np.array([[[1.0, 2.0]]], F32), np.array([[3]], np.uint32)
    tpos = np.zeros((1, m, 2), F32)
    tpos[0, :, 0] = 50.5
    tpos[0, :, 1] = np.arange(m, dtype=np.int64) % 100 + 0.5      # 2^24 tracers over column 50
    tvel = np.zeros((1, m, 2), F32)
    tvel[0, -2:] = [(1.0, 0.5), (2.0, 0.5)]                        # the last two rows, on pixels (14, 50) and (15, 50)
    with nb.RestrictedEnsemble(pos, vel, w, (tpos, tvel)) as ens:
        with pytest.raises(C.NBodyError) as e:
            ens.frames(100, 100, tracers=True)
        assert e.value.code == C.ERR_INVALID and _message(e.value).startswith("restricted frames") and "tracers" in _message(e.value)
        f = ens.frames(100, 100, tracers=False)
        assert np.array_equal(f[0], orc.draw(pos[0], vel[0], w[0], 100, 100))
        ens.set_tracers((tpos[:, 1:], tvel[:, 1:]))              # n + m = 2^24 exactly: the last row is row 2^24 - 1
        g = ens.frames(100, 100, tracers=True)[0]
        assert tuple(g[20, 10]) == (255, 255 - 0x10 - 30, 255 - 0x10 - 30, 10)
        assert (g[:, 50, 3] == 250).all() and (g[:, 50, 0] == 255).all()
        assert g[(m - 1) % 100, 50, 1] == 255 - 0x10 - 25 and g[(m - 2) % 100, 50, 1] == 255 - 0x10 - 15   # the LAST rows' colours
        others = np.ones(100, bool)
        others[[(m - 1) % 100, (m - 2) % 100]] = False
        assert (g[others, 50, 1] == 255 - 0x10).all()
        g[:, 50] = 0
        g[20, 10] = 0
        assert not g.any()
