"""A watched run on the device (watch() of the eight ensemble classes over nbody_watch_*), compared on bytes — no tolerance
anywhere.  The twin test runs two handles of one class on the same worlds: one calls watch(), the other loops over encounters(),
particles() / tracers() and update(delta, 1), and the restatement of the contract (tests/_watch_restatement.py) folds what that
loop saw.  The ballistic test asserts hand-computed numbers on worlds whose bodies weigh nothing and so move on straight lines.
test_ensemble_watch_host.py shows on the CPU that the worlds used here tell the contract's tie rules from their alternatives.
Needs an MI355X.

Shapes (a tile is 256 targets, a source chunk 1024).  Uniform classes: n in {1, 2, 255, 256, 257, 1025} in three worlds.
Restricted classes: m in {0, 1, 257} at n = 257 and n in {1, 1025} at m = 300.  Ragged classes: sizes [1, 2, 257, 64, 1025, 255],
the ragged restricted ones with tracer counts [0, 1, 300, 0, 513, 5]."""
import ctypes

import numpy as np
import pytest

import _encounters_scene as S
import _watch_restatement as W

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
WORLDS = 3
CLAMP = 1.5                                         # the handles' clamp: what limit2=None means
DT = 2.0 ** -10
N_STEPS = 5
HEIGHT = 8                                          # some rows of every kind of world are inside [0, 8)^2 and some are not
RAGGED_N = [1, 2, 257, 64, 1025, 255]
RR_M = [0, 1, 300, 0, 513, 5]

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
            out += [(kind, (257,) * WORLDS, (m,) * WORLDS) for m in (0, 1, 257)]
            out += [(kind, (n,) * WORLDS, (300,) * WORLDS) for n in (1, 1025)]
        else:
            out += [(kind, (n,) * WORLDS, (0,) * WORLDS) for n in (1, 2, 255, 256, 257, 1025)]
    return out


SHAPES = _shapes()
# one shape per class for everything but the twin test: the uniform ones at n = 257 (and m = 257)
ONE_EACH = [s for s in SHAPES if KINDS[s[0]][2] or (s[1][0] == 257 and s[2][0] == (257 if KINDS[s[0]][3] else 0))]


def _id(shape):
    kind, sizes, counts = shape
    return kind if KINDS[kind][2] else f"{kind}-n{sizes[0]}-m{counts[0]}"


def build(nb, kind, bodies, vels, tracers=None, weights=None, **params):
    """The class of `kind` holding these worlds: bodies, vels lists of [n_k, 2]; tracers None or a list of (pos, vel) pairs."""
    cls_name, _, ragged, has_tracers, _ = KINDS[kind]
    cls = getattr(nb, cls_name)
    if ragged:
        if not has_tracers:
            return cls(bodies, vels, weights, **params)
        return cls(bodies, vels, weights, [t if len(t[0]) else None for t in tracers], **params)
    pos, vel = np.stack(bodies), np.stack(vels)
    weights = None if weights is None else np.stack(weights)
    if not has_tracers:
        return cls(pos, vel, weights, **params)
    return cls(pos, vel, weights, (np.stack([t[0] for t in tracers]), np.stack([t[1] for t in tracers])), **params)


class Case:
    """A shape's scene and how to put (some of) its worlds on the device."""

    def __init__(self, nb, shape):
        self.nb, (self.kind, sizes, counts) = nb, shape
        self.cls_name, self.dtype, self.ragged, self.has_tracers, self.who = KINDS[self.kind]
        self.sizes, self.counts = list(sizes), list(counts)
        seed = S.seed_of("watch", self.kind, sizes, counts)
        self.worlds = []
        for k, (n, m) in enumerate(zip(self.sizes, self.counts)):
            pos = S.world(seed, k, n, self.dtype)
            rng = np.random.default_rng([seed, k, 99])
            self.worlds.append(dict(pos=pos, vel=rng.uniform(-1, 1, (n, 2)).astype(self.dtype), tpos=S.tracers(seed, k, m, self.dtype, pos),
                                    tvel=rng.uniform(-1, 1, (m, 2)).astype(self.dtype)))
        self.own = list(range(len(self.sizes)))
        self.limits = S.limits(len(self.own), shift=self.sizes[0] + self.counts[-1])

    def make(self, which=None, **params):
        ws = [self.worlds[k] for k in (self.own if which is None else which)]
        params.setdefault("clamp", CLAMP)
        return build(self.nb, self.kind, [x["pos"] for x in ws], [x["vel"] for x in ws], [(x["tpos"], x["tvel"]) for x in ws], **params)

    def segments(self):
        return (False, True) if self.has_tracers else (False,)

    def watch(self, ens, tracers=False, **kw):
        return ens.watch(DT, tracers=tracers, **kw) if self.has_tracers else ens.watch(DT, **kw)

    def encounters(self, ens, limit2, tracers):
        return ens.encounters(limit2, tracers, True) if self.has_tracers else ens.encounters(limit2, True)

    def targets(self, ens, tracers):
        """-> the per-world positions of the segment's targets as the handle holds them now."""
        if not tracers:
            return list(ens.particles()[0])
        t = ens.tracers()
        return [p for p, _ in t] if self.ragged else list(t[0])

    def state(self, ens):
        """Everything the handle holds, as bytes."""
        p, v, _ = ens.particles()
        out = [np.asarray(a).tobytes() for a in list(p) + list(v)]
        if self.has_tracers:
            t = ens.tracers()
            out += [np.asarray(a).tobytes() for pair in t for a in pair] if self.ragged else [t[0].tobytes(), t[1].tobytes()]
        return out

    def n_targets(self, k, tracers):
        return self.counts[k] if tracers else self.sizes[k]


def _world(got, i):
    """World i of a watch() result -> (record, rows dict)."""
    rec, rows = got
    return rec[i], {name: rows[name][i] for name in W.ROWS}


def _looped(c, ens, limits, n_steps):
    """What the user's loop sees: per segment and world the list of (sample, nn_index, nn_d2, targets), one entry per state after
    0 .. n_steps steps of `ens`, which is stepped by update(DT, 1)."""
    seen = {tr: [[] for _ in c.own] for tr in c.segments()}
    for s in range(n_steps + 1):
        for tr in c.segments():
            _, idx, d2, _ = c.encounters(ens, limits, tr)
            pos = c.targets(ens, tr)
            for i in range(len(c.own)):
                seen[tr][i].append((s, idx[i], d2[i], pos[i]))
        if s < n_steps:
            ens.update(DT)
    return seen


def _check(c, got, seen, which, tracers, limits, samples, what):
    """got: what watch() returned for the worlds `which`; seen: _looped's lists for them; samples: the sample numbers taken."""
    rec, rows = got
    assert rec.dtype == c.nb.WATCH_DTYPE and rec.shape == (len(which),)
    for i, k in enumerate(which):
        want = W.fold([seen[i][s] for s in samples], CLAMP if limits is None else limits[i], HEIGHT, c.n_targets(k, tracers), c.sizes[k], c.dtype)
        mine = _world(got, i) if rows is not None else (rec[i], want[1])
        assert W.same_world(mine, want), f"{what}, world {k} (slot {i}, tracers {tracers}): {W.diff(mine, want)} differ: got {rec[i]}, expected {want[0]}"


@pytest.fixture(params=SHAPES, ids=_id)
def case(request, nb):
    return Case(nb, request.param)


@pytest.fixture(params=ONE_EACH, ids=_id)
def one(request, nb):
    return Case(nb, request.param)


@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_a_watch_is_the_loop_over_encounters_particles_and_update(case, arith):
    c = case
    with c.make(arith=arith) as twin:
        seen = _looped(c, twin, c.limits, N_STEPS)
        final = c.state(twin)
    for k, (stride, tracers) in enumerate((s, t) for s in (1, 2) for t in c.segments()):
        with c.make(arith=arith) as ens:
            got = c.watch(ens, tracers, n_steps=N_STEPS, limit2=c.limits, height=HEIGHT, stride=stride)
            _check(c, got, seen[tracers], c.own, tracers, c.limits, W.taken(N_STEPS, stride), f"stride {stride}")
            rec, rows = got
            assert [int(r) for r in rec["rows"]] == [c.n_targets(k, tracers) for k in c.own] and [int(r) for r in rec["sources"]] == c.sizes
            assert all(a.dtype == (np.dtype(c.dtype) if name == "min_d2" else np.int32 if name == "min_index" else np.uint32)
                       for name in W.ROWS for a in rows[name])
            assert c.state(ens) == final, f"the rows after watch(stride {stride}, tracers {tracers}) are not those after the updates"


@pytest.mark.parametrize("kind", ["ensemble", "rr"])
def test_a_worlds_record_and_rows_are_the_same_alone(nb, kind):
    shape = (kind, (257, 2, 64), (300, 0, 5)) if KINDS[kind][2] else (kind, (257,) * WORLDS, (0,) * WORLDS)
    c = Case(nb, shape)
    for tracers in c.segments():
        with c.make() as ens:
            whole = c.watch(ens, tracers, n_steps=N_STEPS, limit2=c.limits, height=HEIGHT, stride=2)
        for k in c.own:
            with c.make([k]) as ens:
                alone = c.watch(ens, tracers, n_steps=N_STEPS, limit2=c.limits[k:k + 1], height=HEIGHT, stride=2)
            assert W.same_world(_world(alone, 0), _world(whole, k)), (k, tracers, W.diff(_world(alone, 0), _world(whole, k)))


def _raw(c, h, flags, n_steps, stride, limits, height, out, arrays, delta=DT):
    """nbody_watch_<handle> through ctypes: arrays a list of six arrays or None each, or None for rows == NULL."""
    C = c.nb._capi
    call = getattr(C.load(), "nbody_watch_" + c.kind)
    block = None if arrays is None else C.WatchRows(*[None if a is None else a.ctypes.data for a in arrays])
    return call(h.h, flags, delta, n_steps, stride, None if limits is None else limits.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), height,
                None if out is None else C._ptr(out), None if block is None else ctypes.byref(block), None)


def test_the_optional_arrays_change_nothing(one):
    c = one
    for tracers in c.segments():
        flags = 1 if tracers else 0
        with c.make() as ens:
            whole = c.watch(ens, tracers, n_steps=3, limit2=c.limits, height=HEIGHT)
        with c.make() as ens:
            assert W.same(c.watch(ens, tracers, n_steps=3, limit2=c.limits, height=HEIGHT, rows=False)[0], whole[0])
        flat = [np.concatenate([np.ravel(a) for a in whole[1][name]]) for name in W.ROWS]
        for mask in (0, 63, 1, 32, 21, 42, 6, 56):                      # which of the six arrays are asked for, after three steps
            with c.make() as ens:
                out = np.zeros(len(c.own), c.nb.WATCH_DTYPE)
                arrays = [np.zeros_like(f) if mask >> i & 1 else None for i, f in enumerate(flat)]
                ens.h._check(_raw(c, ens.h, flags, 3, 1, c.limits, HEIGHT, out, arrays))
                assert W.same(out, whole[0]), mask
                assert all(a is None or W.same(a, f) for a, f in zip(arrays, flat)), mask
        with c.make() as ens:                                           # every subset, on one sample without a step
            first = c.watch(ens, tracers, n_steps=0, limit2=c.limits, height=HEIGHT)
            flat = [np.concatenate([np.ravel(a) for a in first[1][name]]) for name in W.ROWS]
            for mask in range(65):
                out = np.zeros(len(c.own), c.nb.WATCH_DTYPE)
                arrays = None if mask == 64 else [np.zeros_like(f) if mask >> i & 1 else None for i, f in enumerate(flat)]
                ens.h._check(_raw(c, ens.h, flags, 0, 1, c.limits, HEIGHT, out, arrays))
                assert W.same(out, first[0]), mask
                assert arrays is None or all(a is None or W.same(a, f) for a, f in zip(arrays, flat)), mask


@pytest.mark.parametrize("stride", [1, 2])
def test_a_run_split_over_two_calls_merges_into_the_whole(one, stride):
    c = one
    n1, n2 = 2 * stride, 3
    for tracers in c.segments():
        with c.make() as ens:
            whole = c.watch(ens, tracers, n_steps=n1 + n2, limit2=c.limits, height=HEIGHT, stride=stride)
            final = c.state(ens)
        with c.make() as ens:
            first = c.watch(ens, tracers, n_steps=n1, limit2=c.limits, height=HEIGHT, stride=stride)
            second = c.watch(ens, tracers, n_steps=n2, limit2=c.limits, height=HEIGHT, stride=stride, resume=True)
            assert c.state(ens) == final
        assert list(first[0]["samples"]) == [len(W.taken(n1, stride))] * len(c.own)
        assert list(second[0]["samples"]) == [len(W.taken(n2, stride, True))] * len(c.own)
        merged = c.nb.watch_merge(first, second, n1)
        for i in c.own:
            assert W.same_world(_world(merged, i), _world(whole, i)), (i, tracers, W.diff(_world(merged, i), _world(whole, i)))


def test_no_step_is_one_encounters_sample_and_with_resume_no_sample_at_all(one):
    c = one
    with c.make() as ens:
        before = c.state(ens)
        for tracers in c.segments():
            rec, rows = c.watch(ens, tracers, n_steps=0, limit2=c.limits, height=HEIGHT)
            erec, idx, d2, close = c.encounters(ens, c.limits, tracers)
            for i, k in enumerate(c.own):
                assert W.same(rows["min_index"][i], idx[i]) and W.same(rows["min_d2"][i], d2[i]), (k, tracers)
                assert W.same(rows["close_samples"][i], (close[i] > 0).astype(np.uint32)), (k, tracers)
                assert W.same(rows["min_sample"][i], np.where(idx[i] >= 0, 0, W.NEVER).astype(np.uint32))
                assert rec["samples"][i] == 1 and rec["close_rows"][i] == erec["close_rows"][i] and rec["isolated_rows"][i] == erec["isolated_rows"][i]
                assert (rec["min_row"][i], rec["min_source"][i], rec["min_d2"][i]) == (erec["min_row"][i], erec["min_source"][i], erec["min_d2"][i])
            rec, rows = c.watch(ens, tracers, n_steps=0, limit2=c.limits, height=HEIGHT, resume=True)
            for i, k in enumerate(c.own):
                want = W.fold([], c.limits[i], HEIGHT, c.n_targets(k, tracers), c.sizes[k], c.dtype)
                assert W.same_world(_world((rec, rows), i), want), (k, tracers, W.diff(_world((rec, rows), i), want))
                assert rec["samples"][i] == 0 and rec["isolated_rows"][i] == c.n_targets(k, tracers)
            rec, rows = c.watch(ens, tracers, n_steps=0, limit2=c.limits, height=HEIGHT, resume=True, rows=False)
            assert rows is None and list(rec["samples"]) == [0] * len(c.own)
        assert c.state(ens) == before


def test_the_run_is_an_updates_run(one):
    c = one
    with c.make() as watched, c.make() as stepped:
        counter = c.nb.Counting()
        for tracers in c.segments():
            c.watch(watched, tracers, n_steps=N_STEPS, limit2=c.limits, height=HEIGHT, stride=2, counter=counter)
            stepped.update(DT, n_steps=N_STEPS)
        assert counter.sum_gravity > 0.0 and counter.build_bvh == 0.0 and counter.post_calculations == 0.0
        assert c.state(watched) == c.state(stepped)
        for tracers in c.segments():
            a = watched.deltas(tracers) if c.has_tracers else watched.deltas()
            b = stepped.deltas(tracers) if c.has_tracers else stepped.deltas()
            assert a[1] == b[1] == N_STEPS * len(c.segments())               # the step count advanced by n_steps per call
            assert a[0] == b[0]


def _message(err):
    """The library's own message: NBodyError puts "nbody_hip error <code>: " in front of it."""
    head = f"nbody_hip error {err.code}: "
    assert str(err).startswith(head)
    return str(err)[len(head):]


def test_refusals_name_the_handle_and_watch_and_change_nothing(one, nb):
    c = one
    C = nb._capi
    out = np.zeros(len(c.own), nb.WATCH_DTYPE)

    def refused(h, *words, flags=0, n_steps=1, stride=1, height=0, out_=out):
        with pytest.raises(C.NBodyError) as e:
            h._check(_raw(c, h, flags, n_steps, stride, None, height, out_, None))
        assert e.value.code == C.ERR_INVALID
        msg = _message(e.value)
        assert msg.startswith(c.who + " watch: "), msg
        for w in words:
            assert w in msg, (w, msg)

    empty = getattr(C, HANDLES[c.kind])(0)                            # a handle of the class's kind with nothing uploaded
    try:
        refused(empty, "nothing uploaded")
    finally:
        empty.close()
    with c.make() as ens:
        before = c.state(ens)
        step = (ens.deltas(False, True) if c.has_tracers else ens.deltas(True))[1]
        refused(ens.h, "out is NULL", out_=None)
        refused(ens.h, "unknown flag", flags=4)
        refused(ens.h, "unknown flag", flags=0x80000002)
        if not c.has_tracers:
            refused(ens.h, "NBODY_WATCH_TRACERS", "without tracers", flags=C.WATCH_TRACERS)
        refused(ens.h, "n_steps", n_steps=-1)
        refused(ens.h, "stride", stride=0)
        refused(ens.h, "stride", stride=-3)
        refused(ens.h, "height", "2^24", height=(1 << 24) + 1)
        assert not out.view(np.uint8).any()                             # nothing was written
        assert c.state(ens) == before                                   # and nothing stepped
        assert (ens.deltas(False, True) if c.has_tracers else ens.deltas(True))[1] == step
        for tracers in c.segments():                                    # and the handle works
            rec, _ = c.watch(ens, tracers, n_steps=1, height=1 << 24)
            assert list(rec["samples"]) == [2] * len(c.own)


@pytest.mark.parametrize("kind", ["ensemble", "ensemble64", "restricted"])
def test_weightless_bodies_on_straight_lines_give_the_hand_computed_numbers(nb, kind):
    """tests/_watch_restatement.py HAND: every body weighs 0, so every force term is +-0 and under EXACT the rows move on
    straight lines through dyadic points: the minimum at a middle sample, the tie in time, the body that leaves the frame at a
    known sample, the one that begins outside and comes in (first_out stays), the pair that is close at exactly two samples.
    (A straight line cannot leave a square and come back: the row that is out first and inside later is what shows that coming
    back does not clear first_out.)"""
    dtype, has_tracers = KINDS[kind][1], KINDS[kind][3]
    h = W.HAND
    pos, vel, tpos, tvel = W.hand_world(dtype)
    weight = [np.zeros(pos.shape[0], np.uint32)]
    for tracers in ((False, True) if has_tracers else (False,)):
        with build(nb, kind, [pos], [vel], [(tpos, tvel)], weight, clamp=h["limit2"], arith="exact") as ens:
            kw = dict(tracers=tracers) if has_tracers else {}
            rec, rows = ens.watch(h["delta"], n_steps=h["n_steps"], height=h["height"], **kw)      # limit2 None: the clamp
            want = W.hand_expected("tracers" if tracers else "bodies", dtype)
            got = _world((rec, rows), 0)
            for name in W.ROWS:                                        # the numbers themselves
                assert list(got[1][name]) == list(want[1][name]), (name, tracers)
            for name in W.DTYPE.names:
                assert got[0][name] == want[0][name], (name, tracers)
            assert W.same_world(got, want)
            p = ens.particles()[0][0]
            assert W.same(p, W.ballistic(pos, vel, h["delta"], h["n_steps"])[-1])                 # straight lines indeed
            if has_tracers:
                assert W.same(ens.tracers()[0][0], W.ballistic(tpos, tvel, h["delta"], h["n_steps"])[-1])


@pytest.mark.parametrize("kind", ["ensemble", "ensemble64"])
def test_the_lattice_at_rest_keeps_the_earliest_sample_and_the_lowest_source(nb, kind):
    """The world test_ensemble_watch_host.py shows to tell the tie rules apart: every minimum tied over all samples, most of
    them tied between sources."""
    dtype = KINDS[kind][1]
    pos, vel = W.static_lattice(dtype)
    with build(nb, kind, [pos], [vel], None, [np.zeros(pos.shape[0], np.uint32)], clamp=CLAMP, arith="exact") as ens:
        got = _world(ens.watch(0.5, n_steps=N_STEPS, height=HEIGHT), 0)
        assert W.same(ens.particles()[0][0], pos)
    frames = W.frames_of(W.taken(N_STEPS), [pos] * (N_STEPS + 1))
    want = W.world(frames, CLAMP, HEIGHT, pos.shape[0], pos.shape[0], dtype)
    assert W.same_world(got, want), W.diff(got, want)
    for rival in (dict(latest=True), dict(highest=True)):
        other = W.world(frames, CLAMP, HEIGHT, pos.shape[0], pos.shape[0], dtype, **rival)
        assert not W.same_world(got, other)
