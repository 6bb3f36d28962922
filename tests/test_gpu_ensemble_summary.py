"""Summaries of an ensemble on the device (summary() of the eight ensemble classes over nbody_summary_*): every world's record
against nb.summary_of of that world's own rows and against the NumPy restatement of the contract (tests/_summary_restatement.py),
compared on the record's bytes — no tolerance anywhere; a NaN field matches any NaN.  The scene is tests/_summary_scene.py: its
coordinates span 70 binades, so another order of additions gives other bits (test_ensemble_summary_host.py asserts that on the
CPU for these very rows), and it plants NaN, +-inf, signed zeros as extreme values, weights that round in f32 and, in one f64
world, a velocity whose square overflows.  Needs an MI355X.

Shapes.  Uniform classes: n in {1, 256, 257, 600, 4096} (a lane's stride over rows is 256; 4096 fills the chunk), four worlds.
Restricted classes: m in {0, 300, 4097, 9000} at n = 257 (one, two and three chunks of tracers) and every n at m = 300.  Ragged
classes: sizes [1, 2, 257, 64, 600, 4096, 255], the ragged restricted ones with tracer counts [0, 1, 300, 0, 4097, 9000, 5].  The
reference-world cases of the ragged classes add two worlds, of 257 and 600 bodies (300 and 4097 tracers), because a reference
must have the rows of the world measured from it and the seven sizes are all different."""
import numpy as np
import pytest

import _summary_restatement as R
import _summary_scene as S

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
W = 4
H = S.HEIGHT
DT = 2.0 ** -10
RAGGED_N = [1, 2, 257, 64, 600, 4096, 255]
RR_M = [0, 1, 300, 0, 4097, 9000, 5]
TWINS_N, TWINS_M = [257, 600], [300, 4097]      # worlds 7 and 8 of the reference cases: the sizes of worlds 2 and 4

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


HANDLES = {"ensemble": "EnsembleHandle", "ensemble64": "Ensemble64Handle", "ragged": "RaggedHandle", "ragged64": "Ragged64Handle",
           "restricted": "RestrictedHandle", "restricted64": "Restricted64Handle", "rr": "RRHandle", "rr64": "RR64Handle"}


def _shapes():
    out = []
    for kind, (_, _, ragged, tracers, _) in KINDS.items():
        if ragged:
            out.append((kind, tuple(RAGGED_N), tuple(RR_M) if tracers else (0,) * len(RAGGED_N)))
        elif tracers:
            out += [(kind, (257,) * W, (m,) * W) for m in (0, 300, 4097, 9000)]
            out += [(kind, (n,) * W, (300,) * W) for n in (1, 256, 600, 4096)]
        else:
            out += [(kind, (n,) * W, (0,) * W) for n in (1, 256, 257, 600, 4096)]
    return out


SHAPES = _shapes()
# one shape per class for the refusals: the uniform ones at n = 257 (and m = 300)
ONE_EACH = [s for s in SHAPES if KINDS[s[0]][2] or (s[1][0] == 257 and s[2][0] == (300 if KINDS[s[0]][3] else 0))]


def _id(shape):
    kind, sizes, counts = shape
    return kind if KINDS[kind][2] else f"{kind}-n{sizes[0]}-m{counts[0]}"


class Case:
    """A shape's scene and how to put (some of) its worlds on the device."""

    def __init__(self, nb, shape):
        self.nb, (self.kind, sizes, counts) = nb, shape
        self.cls_name, self.dtype, self.ragged, self.has_tracers, self.who = KINDS[self.kind]
        self.sizes, self.counts = list(sizes), list(counts)
        if self.ragged:  # the twins go last: worlds 0 .. 6 are the shape's own
            self.all_sizes, self.all_counts = self.sizes + TWINS_N, self.counts + (TWINS_M if self.has_tracers else [0, 0])
        else:
            self.all_sizes, self.all_counts = self.sizes, self.counts
        self.worlds = S.scene(self.all_sizes, self.all_counts, self.dtype)
        self.own = list(range(len(self.sizes)))
        self._expected = {}

    def make(self, which=None):
        """The class's ensemble of the worlds `which` (default: the shape's own)."""
        ws = [self.worlds[k] for k in (self.own if which is None else which)]
        cls = getattr(self.nb, self.cls_name)
        pos, vel, w = [x["pos"] for x in ws], [x["vel"] for x in ws], [x["w"] for x in ws]
        if self.ragged:
            if not self.has_tracers:
                return cls(pos, vel, w)
            return cls(pos, vel, w, [(x["tpos"], x["tvel"]) if len(x["tpos"]) else None for x in ws])
        pos, vel, w = np.stack(pos), np.stack(vel), np.stack(w)
        if not self.has_tracers:
            return cls(pos, vel, w)
        return cls(pos, vel, w, (np.stack([x["tpos"] for x in ws]), np.stack([x["tvel"] for x in ws])))

    def segments(self):
        return (False, True) if self.has_tracers else (False,)

    def summary(self, ens, tracers=False, ref=None, height=H):
        return ens.summary(height, ref, tracers) if self.has_tracers else ens.summary(height, ref)

    def rows(self, k, tracers, state=None):
        """-> (pos, vel, weight or None) of world k's addressed segment, as uploaded or as `state` holds it."""
        x = self.worlds[k] if state is None else state[k]
        return (x["tpos"], x["tvel"], None) if tracers else (x["pos"], x["vel"], self.worlds[k]["w"])

    def state(self, ens, which=None):
        """-> {world: dict(pos, vel, tpos, tvel)} as the handle holds the worlds `which` now."""
        which = self.own if which is None else which
        p, v, _ = ens.particles()
        empty = np.zeros((0, 2), self.dtype)
        out = {}
        t = ens.tracers() if self.has_tracers else None
        for i, k in enumerate(which):
            if not self.has_tracers:
                tp, tv = empty, empty
            elif self.ragged:
                tp, tv = t[i]
            else:
                tp, tv = t[0][i], t[1][i]
            out[k] = dict(pos=p[i], vel=v[i], tpos=tp, tvel=tv)
        return out

    def expected(self, k, tracers, j=-1, state=None):
        """World k's record measured from world j (-1: no reference) by nb.summary_of, checked against the restatement; of the
        scene as uploaded it is computed once and shared."""
        key = (k, bool(tracers), j)
        if state is None and key in self._expected:
            return self._expected[key]
        pos, vel, w = self.rows(k, tracers, state)
        ref = None if j < 0 else self.rows(j, tracers, state)[:2]
        got = self.nb.summary_of(pos, vel, w, ref, H)
        want = R.record(pos, vel, w, ref, H)
        assert R.same(got, want), f"summary_of and the restatement differ in {R.diff(got, want)} (world {k}, tracers {tracers}, ref {j})"
        if state is None:
            self._expected[key] = got
        return got


def _same(got, want, what):
    assert R.same(got, want), f"{what}: {R.diff(got, want)} differ: got {got}, expected {want}"


def _check(c, got, which, tracers, ref=None, state=None, what=""):
    assert got.dtype == c.nb.SUMMARY_DTYPE and got.shape == (len(which),)
    for i, k in enumerate(which):
        j = -1 if ref is None or ref[i] < 0 else which[ref[i]]
        _same(got[i], c.expected(k, tracers, j, state), f"{what} world {k} (slot {i}, tracers {tracers}, ref {j})")


def _message(err):
    """The library's own message: NBodyError puts "nbody_hip error <code>: " in front of it."""
    head = f"nbody_hip error {err.code}: "
    assert str(err).startswith(head)
    return str(err)[len(head):]


@pytest.fixture(scope="module", params=SHAPES, ids=_id)
def case(request, nb):
    c = Case(nb, request.param)
    c.ens = c.make()          # shared by the tests that only look; never stepped
    yield c
    c.ens.close()


@pytest.fixture(params=ONE_EACH, ids=_id)
def one(request, nb):
    """One shape per class, for the refusals."""
    return Case(nb, request.param)


def test_every_worlds_record_is_summary_of_its_own_rows(case):
    c = case
    for tracers in c.segments():
        got = c.summary(c.ens, tracers)
        _check(c, got, c.own, tracers, what="all worlds")
        assert [int(r) for r in got["rows"]] == (c.counts if tracers else c.sizes)
        assert not got["sep_rows"].any() and not got["sep_max2"].any() and not got["sep_sum2"].any()
        assert not np.signbit(got["sep_max2"]).any() and not np.signbit(got["sep_sum2"]).any()
        zero = c.summary(c.ens, tracers, height=0)
        assert not zero["in_bounds"].any()
        for name in R.DTYPE.names:
            if name != "in_bounds":
                assert R.same(R.only(zero, name), R.only(got, name)), name     # the frame moves nothing else


def test_a_worlds_record_is_the_same_alone_and_with_the_worlds_reversed(case):
    c = case
    back = c.own[::-1]
    with c.make(back) as ens:
        for tracers in c.segments():
            _check(c, c.summary(ens, tracers), back, tracers, what="reversed")
    for k in c.own:
        with c.make([k]) as ens:
            for tracers in c.segments():
                _check(c, c.summary(ens, tracers), [k], tracers, what="alone")


def test_separations_from_itself_from_another_world_from_none_and_mixed(case):
    c = case
    if c.ragged:
        which = c.own + [len(c.own), len(c.own) + 1]
        ens = c.make(which)
        other = np.full(len(which), -1, np.int32)
        other[[2, 7, 4, 8]] = [7, 2, 8, 4]                              # the twins; the other worlds have no world of their size
        if c.has_tracers:
            other[[0, 3]] = [3, 0]                                      # (two worlds without tracers are of one size, too: 0 rows)
    else:
        which, ens = c.own, c.ens
        other = np.array([1, 2, 3, 0], np.int32)
    n = len(which)
    itself = np.arange(n, dtype=np.int32)
    try:
        for tracers in c.segments():
            ref = other.copy()
            if c.ragged and not tracers:
                ref[[0, 3]] = -1                                        # (as bodies worlds 0 and 3 differ in size)
            mix = ref.copy()
            mix[0], mix[n - 1] = 0, -1                                  # itself, others and none in one call
            got = c.summary(ens, tracers, itself)
            _check(c, got, which, tracers, itself, what="ref itself")
            assert np.array_equal(got["sep_rows"], got["counted"])
            assert not got["sep_max2"].any() and not np.signbit(got["sep_max2"]).any() and not got["sep_sum2"].any()
            _check(c, c.summary(ens, tracers, ref), which, tracers, ref, what="ref another")
            none = c.summary(ens, tracers, np.full(n, -1, np.int32))
            _check(c, none, which, tracers, what="ref -1")
            assert R.same(none, c.summary(ens, tracers, None))
            _check(c, c.summary(ens, tracers, mix), which, tracers, mix, what="ref mixed")
    finally:
        if ens is not c.ens:
            ens.close()


def test_after_an_update_and_after_a_sweep_it_is_summary_of_the_download(case):
    c = case
    n = len(c.own)
    ref = None if c.ragged else np.array([1, 2, 3, 0], np.int32)
    with c.make() as ens:
        ens.update(DT)
        state = c.state(ens)
        for tracers in c.segments():
            _check(c, c.summary(ens, tracers, ref), c.own, tracers, ref, state, what="after update")
        ens.sweep(np.array([DT * (k + 1) for k in range(n)], c.dtype), steps=np.arange(n) % 3, n_steps=2)
        state = c.state(ens)
        for tracers in c.segments():
            _check(c, c.summary(ens, tracers, ref), c.own, tracers, ref, state, what="after sweep")


def test_step_summary_step_gives_the_bits_of_step_step(case):
    c = case
    with c.make() as a, c.make() as b:
        a.update(DT)
        for tracers in c.segments():
            c.summary(a, tracers, np.zeros(len(c.own), np.int32) if not c.ragged else None)
        a.update(DT)
        b.update(DT, n_steps=2)
        sa, sb = c.state(a), c.state(b)
        for k in c.own:
            for name in ("pos", "vel", "tpos", "tvel"):
                assert np.array_equal(sa[k][name].view(np.uint8), sb[k][name].view(np.uint8)), (k, name)


def test_refusals_name_the_handle_and_summary_and_leave_the_handle_working(one, nb):
    c = one
    C = nb._capi
    n = len(c.own)
    call = getattr(C.load(), "nbody_summary_" + c.kind)
    out = np.zeros(n, nb.SUMMARY_DTYPE)

    def refused(h, fn, *words):
        with pytest.raises(C.NBodyError) as e:
            fn()
        assert e.value.code == C.ERR_INVALID
        msg = _message(e.value)
        assert msg.startswith(c.who + " summary: "), msg
        for w in words:
            assert w in msg, (w, msg)

    def raw(h, flags, height, ref, out_ptr):
        h._check(call(h.h, flags, height, ref, out_ptr))

    empty = getattr(C, HANDLES[c.kind])(0)                            # a handle of the class's kind with nothing uploaded
    try:
        refused(empty, lambda: raw(empty, 0, H, None, C._ptr(out)), "nothing uploaded")
    finally:
        empty.close()
    with c.make() as ens:
        h = ens.h
        refused(h, lambda: raw(h, 0, H, None, None), "out is NULL")
        refused(h, lambda: raw(h, 2, H, None, C._ptr(out)), "unknown flag")
        refused(h, lambda: raw(h, 0x80000001, H, None, C._ptr(out)), "unknown flag")
        if not c.has_tracers:
            refused(h, lambda: raw(h, C.SUMMARY_TRACERS, H, None, C._ptr(out)), "NBODY_SUMMARY_TRACERS", "without tracers")
        refused(h, lambda: h.summary((1 << 24) + 1, None), "height", "2^24")
        for bad in (n, -2, 1 << 30):
            ref = np.full(n, -1, np.int32)
            ref[n - 2] = bad
            refused(h, lambda: h.summary(H, ref), f"ref[{n - 2}] = {bad}", f"world {n - 2}", "outside")
        if c.ragged:
            ref = np.full(n, -1, np.int32)
            ref[4] = 5                                                  # 600 rows measured from 4096 (tracers: 4097 from 9000)
            for tracers in c.segments():
                refused(h, lambda: h.summary(H, ref, tracers), "ref[4] = 5", "world 4", "rows")
        assert not out.view(np.uint8).any()                             # nothing was written
        for tracers in c.segments():                                    # and the handle works
            _check(c, c.summary(ens, tracers), c.own, tracers, what="after the refusals")
        big = c.summary(ens, False, height=1 << 24)                     # the largest frame is taken
        _same(big[0], nb.summary_of(*c.rows(c.own[0], False), None, 1 << 24), "height 2^24")
