"""Encounters of an ensemble on the device (encounters() of the eight ensemble classes over nbody_encounters_*): every world's
record and rows against nb.encounters_of of that world's own rows and against the NumPy restatement of the contract
(tests/_encounters_restatement.py), compared on bytes — no tolerance anywhere.  The scene is tests/_encounters_scene.py: a world
with the contract's edges planted in it, an integer lattice full of exact ties and an edge world (one body; two bodies whose d2
overflows); test_ensemble_encounters_host.py asserts on the CPU, for these very kinds of rows, that another tie rule gives other
indices and a fused d2 other bits.  Needs an MI355X.

Shapes.  Uniform classes: n in {1, 2, 64, 65, 256, 257, chunk + 1, 4096} in three worlds (a tile is 256 targets, a source chunk
1024).  Restricted classes: m in {0, 1, 255, 257, 4097} at n = 257 and n in {1, chunk + 1, 4096} at m = 300.  Ragged classes:
sizes [1, 2, 257, 64, chunk + 1, 4096, 255], the ragged restricted ones with tracer counts [0, 1, 300, 0, 4097, 9000, 5]."""
import numpy as np
import pytest

import _encounters_restatement as R
import _encounters_scene as S

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
W = 3
CLAMP = 1.5                                         # the handles' clamp: what limit2=None means
DT = 2.0 ** -10
RAGGED_N = [1, 2, 257, 64, R.CHUNK + 1, 4096, 255]
RR_M = [0, 1, 300, 0, 4097, 9000, 5]

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
            out += [(kind, (257,) * W, (m,) * W) for m in (0, 1, 255, 257, 4097)]
            out += [(kind, (n,) * W, (300,) * W) for n in (1, R.CHUNK + 1, 4096)]
        else:
            out += [(kind, (n,) * W, (0,) * W) for n in (1, 2, 64, 65, 256, 257, R.CHUNK + 1, 4096)]
    return out


SHAPES = _shapes()
# one shape per class for the refusals and the step: the uniform ones at n = 257 (and m = 257)
ONE_EACH = [s for s in SHAPES if KINDS[s[0]][2] or (s[1][0] == 257 and s[2][0] == (257 if KINDS[s[0]][3] else 0))]


def _id(shape):
    kind, sizes, counts = shape
    return kind if KINDS[kind][2] else f"{kind}-n{sizes[0]}-m{counts[0]}"


def build(nb, kind, bodies, vels, tracers=None, **params):
    """The class of `kind` holding these worlds: bodies, vels lists of [n_k, 2]; tracers None or a list of (pos, vel) pairs."""
    cls_name, _, ragged, has_tracers, _ = KINDS[kind]
    cls = getattr(nb, cls_name)
    if ragged:
        if not has_tracers:
            return cls(bodies, vels, None, **params)
        return cls(bodies, vels, None, [t if len(t[0]) else None for t in tracers], **params)
    pos, vel = np.stack(bodies), np.stack(vels)
    if not has_tracers:
        return cls(pos, vel, None, **params)
    return cls(pos, vel, None, (np.stack([t[0] for t in tracers]), np.stack([t[1] for t in tracers])), **params)


class Case:
    """A shape's scene and how to put (some of) its worlds on the device."""

    def __init__(self, nb, shape):
        self.nb, (self.kind, sizes, counts) = nb, shape
        self.cls_name, self.dtype, self.ragged, self.has_tracers, self.who = KINDS[self.kind]
        self.sizes, self.counts = list(sizes), list(counts)
        seed = S.seed_of("gpu", self.kind, sizes, counts)
        self.worlds = []
        for k, (n, m) in enumerate(zip(self.sizes, self.counts)):
            pos = S.world(seed, k, n, self.dtype)
            rng = np.random.default_rng([seed, k, 99])
            self.worlds.append(dict(pos=pos, vel=rng.uniform(-1, 1, (n, 2)).astype(self.dtype), tpos=S.tracers(seed, k, m, self.dtype, pos),
                                    tvel=rng.uniform(-1, 1, (m, 2)).astype(self.dtype)))
        self.own = list(range(len(self.sizes)))
        self.limits = S.limits(len(self.own), shift=self.sizes[0] + self.counts[-1])
        self._expected = {}

    def make(self, which=None, **params):
        ws = [self.worlds[k] for k in (self.own if which is None else which)]
        params.setdefault("clamp", CLAMP)
        return build(self.nb, self.kind, [x["pos"] for x in ws], [x["vel"] for x in ws], [(x["tpos"], x["tvel"]) for x in ws], **params)

    def segments(self):
        return (False, True) if self.has_tracers else (False,)

    def encounters(self, ens, limit2=None, tracers=False, rows=True):
        return ens.encounters(limit2, tracers, rows) if self.has_tracers else ens.encounters(limit2, rows)

    def state(self, ens, which=None):
        """-> {world: dict(pos, vel, tpos, tvel)} as the handle holds the worlds `which` now."""
        which = self.own if which is None else which
        p, v, _ = ens.particles()
        empty = np.zeros((0, 2), self.dtype)
        t = ens.tracers() if self.has_tracers else None
        out = {}
        for i, k in enumerate(which):
            if not self.has_tracers:
                tp, tv = empty, empty
            elif self.ragged:
                tp, tv = t[i]
            else:
                tp, tv = t[0][i], t[1][i]
            out[k] = dict(pos=p[i], vel=v[i], tpos=tp, tvel=tv)
        return out

    def expected(self, k, tracers, limit, state=None):
        """World k's segment under `limit` (a float32) by nb.encounters_of, checked against the restatement; of the scene as
        uploaded it is computed once and shared."""
        key = (k, bool(tracers), np.float32(limit).tobytes())
        if state is None and key in self._expected:
            return self._expected[key]
        x = self.worlds[k] if state is None else state[k]
        targets, sources = (x["tpos"], x["pos"]) if tracers else (x["pos"], None)
        lim = self.dtype(np.float32(limit))                              # widened on the f64 handles
        got = self.nb.encounters_of(targets, sources, lim)
        want = R.segment(targets, sources, lim)
        assert R.same_segment(got, want), f"encounters_of and the restatement differ in {R.diff(got, want)} (world {k}, tracers {tracers})"
        if state is None:
            self._expected[key] = got
        return got


def _check(c, got, which, tracers, limits, state=None, what=""):
    """got: what encounters() returned for the worlds `which` under limits (None: the clamp in every world)."""
    rec, idx, d2, close = got
    assert rec.dtype == c.nb.ENCOUNTERS_DTYPE and rec.shape == (len(which),)
    for i, k in enumerate(which):
        want = c.expected(k, tracers, CLAMP if limits is None else limits[i], state)
        mine = (rec[i], idx[i], d2[i], close[i]) if idx is not None else (rec[i],)
        assert all(R.same(g, w) for g, w in zip(mine, want)), \
            f"{what} world {k} (slot {i}, tracers {tracers}): {R.diff(mine + want[len(mine):], want)} differ: got {rec[i]}, expected {want[0]}"


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
    """One shape per class, for the refusals and the steps."""
    return Case(nb, request.param)


def test_every_worlds_record_and_rows_are_encounters_of_its_own_rows(case):
    c = case
    for tracers in c.segments():
        got = c.encounters(c.ens, c.limits, tracers)
        _check(c, got, c.own, tracers, c.limits, what="all worlds")
        rec, idx, d2, close = got
        assert [int(r) for r in rec["rows"]] == (c.counts if tracers else c.sizes) and [int(r) for r in rec["sources"]] == c.sizes
        per_world = [(a.shape[0], a.dtype) for a in d2] if c.ragged else [(d2.shape[1], d2.dtype)] * len(c.own)
        assert per_world == [(int(r), np.dtype(c.dtype)) for r in rec["rows"]]
        assert all(a.dtype == np.int32 for a in idx) and all(a.dtype == np.uint32 for a in close)
        # limit2 = None is the clamp in every world
        clamp = c.encounters(c.ens, None, tracers)
        _check(c, clamp, c.own, tracers, None, what="limit2 None")
        full = c.encounters(c.ens, np.full(len(c.own), CLAMP, np.float32), tracers)
        assert R.same(clamp[0], full[0]) and all(R.same(a, b) for x, y in zip(clamp[1:], full[1:]) for a, b in zip(x, y))


def test_a_worlds_bytes_are_the_same_alone_reversed_and_without_the_optional_arrays(case):
    c = case
    back = c.own[::-1]
    with c.make(back) as ens:
        for tracers in c.segments():
            _check(c, c.encounters(ens, c.limits[::-1].copy(), tracers), back, tracers, c.limits[::-1], what="reversed")
            _check(c, c.encounters(ens, c.limits[::-1].copy(), tracers, rows=False), back, tracers, c.limits[::-1], what="reversed, records only")
    for k in c.own:
        with c.make([k]) as ens:
            for tracers in c.segments():
                _check(c, c.encounters(ens, c.limits[k:k + 1], tracers), [k], tracers, c.limits[k:k + 1], what="alone")
    for tracers in c.segments():                    # every subset of the optional arrays, through the C call
        C = c.nb._capi
        call = getattr(C.load(), "nbody_encounters_" + c.kind)
        whole = c.encounters(c.ens, c.limits, tracers)
        flat = [np.concatenate([np.ravel(a) for a in x]) if len(x) else np.zeros(0) for x in whole[1:]]
        for mask in range(8):
            out = np.zeros(len(c.own), c.nb.ENCOUNTERS_DTYPE)
            arrays = [np.zeros_like(f) if mask >> i & 1 else None for i, f in enumerate(flat)]
            c.ens.h._check(call(c.ens.h.h, 1 if tracers else 0, c.limits.ctypes.data_as(C.C.POINTER(C.C.c_float)), C._ptr(out),
                                *[C._ptr(a) for a in arrays]))
            assert R.same(out, whole[0]), mask
            assert all(a is None or R.same(a, f) for a, f in zip(arrays, flat)), mask


def test_step_encounters_step_gives_the_bits_of_step_step_and_the_call_sees_the_new_rows(one):
    c = one
    with c.make() as a, c.make() as b:
        a.update(DT)
        state = c.state(a)
        for tracers in c.segments():
            _check(c, c.encounters(a, c.limits, tracers), c.own, tracers, c.limits, state, what="after update")
        a.update(DT)
        b.update(DT, n_steps=2)
        sa, sb = c.state(a), c.state(b)
        for k in c.own:
            for name in ("pos", "vel", "tpos", "tvel"):
                assert np.array_equal(sa[k][name].view(np.uint8), sb[k][name].view(np.uint8)), (k, name)


def test_refusals_name_the_handle_and_encounters_and_leave_the_handle_working(one, nb):
    c = one
    C = nb._capi
    n = len(c.own)
    call = getattr(C.load(), "nbody_encounters_" + c.kind)
    out = np.zeros(n, nb.ENCOUNTERS_DTYPE)

    def refused(fn, *words):
        with pytest.raises(C.NBodyError) as e:
            fn()
        assert e.value.code == C.ERR_INVALID
        msg = _message(e.value)
        assert msg.startswith(c.who + " encounters: "), msg
        for w in words:
            assert w in msg, (w, msg)

    def raw(h, flags, out_ptr):
        h._check(call(h.h, flags, None, out_ptr, None, None, None))

    empty = getattr(C, HANDLES[c.kind])(0)                            # a handle of the class's kind with nothing uploaded
    try:
        refused(lambda: raw(empty, 0, C._ptr(out)), "nothing uploaded")
    finally:
        empty.close()
    with c.make() as ens:
        h = ens.h
        refused(lambda: raw(h, 0, None), "out is NULL")
        refused(lambda: raw(h, 2, C._ptr(out)), "unknown flag")
        refused(lambda: raw(h, 0x80000001, C._ptr(out)), "unknown flag")
        if not c.has_tracers:
            refused(lambda: raw(h, C.ENCOUNTERS_TRACERS, C._ptr(out)), "NBODY_ENCOUNTERS_TRACERS", "without tracers")
        assert not out.view(np.uint8).any()                             # nothing was written
        for tracers in c.segments():                                    # and the handle works
            _check(c, c.encounters(ens, c.limits, tracers), c.own, tracers, c.limits, what="after the refusals")


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_clamp_alters_a_step_exactly_where_close_pairs_says(nb, kind):
    """Two worlds of two bodies, d2 = 0.5 and d2 = 8, under EXACT: with the clamp at 1 the first world's two ordered pairs are
    close and the second's are not; with the clamp at 0.125 none is.  The accelerations and a step differ between the two clamps
    in exactly the world, and for the tracers in exactly the rows, where the call counts close pairs."""
    dtype, has_tracers = KINDS[kind][1], KINDS[kind][3]
    bodies = [np.array([[0, 0], [0.5, 0.5]], dtype), np.array([[0, 0], [2, 2]], dtype)]
    vels = [np.zeros((2, 2), dtype)] * 2
    tpos = np.array([[0.25, 0.5], [5, 5]], dtype)                       # near both bodies of world 0; far from everything
    tracers = [(tpos, np.zeros((2, 2), dtype))] * 2
    seen = {}
    for clamp in (1.0, 0.125):
        with build(nb, kind, bodies, vels, tracers, clamp=clamp, arith="exact") as ens:
            rec = ens.encounters()[0]
            trec, _, _, tclose = ens.encounters(tracers=True) if has_tracers else (None, None, None, None)
            acc = ens.accel()
            tacc = ens.tracers_accel() if has_tracers else None
            ens.update(DT)
            seen[clamp] = (rec, [np.asarray(a) for a in acc], ens.particles()[1], trec, tclose, tacc)
    hi, lo = seen[1.0], seen[0.125]
    assert list(hi[0]["close_pairs"]) == [2, 0] and list(lo[0]["close_pairs"]) == [0, 0]
    assert list(hi[0]["live_pairs"]) == [2, 2] and [float(v) for v in hi[0]["min_d2"]] == [0.5, 8.0]
    for k in range(2):
        altered = bool(hi[0]["close_pairs"][k])
        for a, b in ((hi[1][k], lo[1][k]), (hi[2][k], lo[2][k])):      # accelerations, and the velocities after a step
            differ = np.asarray(a).view(np.uint8) != np.asarray(b).view(np.uint8)
            assert differ.any() == altered, k
            if altered:
                assert (np.asarray(a) != np.asarray(b)).all(), k        # both bodies, both components
    if has_tracers:
        # world 0: the first tracer is at d2 = 0.3125 and 0.0625 from the two bodies; world 1: at 0.3125 and 5.3125
        assert [list(x) for x in hi[4]] == [[2, 0], [1, 0]] and [list(x) for x in lo[4]] == [[1, 0], [0, 0]]
        assert list(hi[3]["close_pairs"]) == [2, 1] and list(lo[3]["close_pairs"]) == [1, 0]
        for k in range(2):
            for r in range(2):
                altered = hi[4][k][r] > 0                               # a pair clamped to 1: unclamped, or clamped to 0.125, under the other
                differ = (np.asarray(hi[5][k][r]).view(np.uint8) != np.asarray(lo[5][k][r]).view(np.uint8)).any()
                assert differ == altered, (k, r)
