"""A watched sweep on the device (watch_sweep() of the eight ensemble classes over nbody_wsweep_*), compared on bytes — no
tolerance anywhere.  The contract is per world: world k's record and rows are those of a one-world handle of the same class with
clamp[k] that calls watch(delta[k], steps[k], stride=stride[k]), and the state afterwards is a sweep's.  The twin test restates
it without watch(): a second handle is stepped by sweep(..., n_steps=1) with encounters() and particles() in between, and the
restatement (tests/_watch_restatement.py) folds what that loop saw at each world's own taken samples.
test_ensemble_wsweep_host.py shows on the CPU that these worlds and parameters (tests/_wsweep_scene.py) tell the contract from
its neighbours: another world's stride, params.clamp as the default limit, sampling on after steps[k], a launch-wide `first`.
Needs an MI355X.

Shapes (a tile is 256 targets, a source chunk 1024), six worlds each.  Uniform classes: n in {1, 2, 257, 1025}.  Restricted
classes: (n = 257, m in {0, 257}) and (n = 1025, m = 300).  Ragged classes: sizes [1, 2, 257, 64, 1025, 255], the ragged
restricted ones with tracer counts [0, 1, 300, 0, 513, 5]."""
import ctypes

import numpy as np
import pytest

import _watch_restatement as W
import _wsweep_scene as Q
from _wsweep_scene import CLAMP, DELTA, HEIGHT, KINDS, N_STEPS, PARAM_CLAMP, STEPS, STRIDE, WORLDS

pytestmark = pytest.mark.gpu
HANDLES = {"ensemble": "EnsembleHandle", "ensemble64": "Ensemble64Handle", "ragged": "RaggedHandle", "ragged64": "Ragged64Handle",
           "restricted": "RestrictedHandle", "restricted64": "Restricted64Handle", "rr": "RRHandle", "rr64": "RR64Handle"}


def _shapes():
    out = []
    for kind, (_, _, ragged, tracers, _) in KINDS.items():
        if ragged:
            out.append((kind, tuple(Q.RAGGED_N), tuple(Q.RR_M) if tracers else (0,) * WORLDS))
        elif tracers:
            out += [(kind, (n,) * WORLDS, (m,) * WORLDS) for n, m in ((257, 0), (257, 257), (1025, 300))]
        else:
            out += [(kind, (n,) * WORLDS, (0,) * WORLDS) for n in (1, 2, 257, 1025)]
    return out


SHAPES = _shapes()
# one shape per class: the uniform ones at n = 257 (and m = 257)
ONE_EACH = [s for s in SHAPES if KINDS[s[0]][2] or (s[1][0] == 257 and s[2][0] == (257 if KINDS[s[0]][3] else 0))]


def _id(shape):
    kind, sizes, counts = shape
    return kind if KINDS[kind][2] else f"{kind}-n{sizes[0]}-m{counts[0]}"


class Case:
    """A shape's scene and how to put (some of) its worlds on the device."""

    def __init__(self, nb, shape):
        self.nb, (self.kind, sizes, counts) = nb, shape
        self.cls_name, self.dtype, self.ragged, self.has_tracers, self.who = KINDS[self.kind]
        self.sizes, self.counts = list(sizes), list(counts)
        self.worlds, self.limits = Q.scene(self.kind, self.sizes, self.counts)
        self.own = list(range(WORLDS))
        self.delta = DELTA.astype(self.dtype)

    def make(self, which=None, **params):
        ws = [self.worlds[k] for k in (self.own if which is None else which)]
        params.setdefault("clamp", PARAM_CLAMP)
        return Q.build(self.nb, self.kind, [x["pos"] for x in ws], [x["vel"] for x in ws], [(x["tpos"], x["tvel"]) for x in ws], **params)

    def segments(self):
        return (False, True) if self.has_tracers else (False,)

    def wsweep(self, ens, tracers=False, which=None, limit2=None, **kw):
        """watch_sweep of the worlds `which` (all) under the scene's parameters, each of which a keyword replaces."""
        sel = self.own if which is None else which
        args = dict(delta=self.delta[sel], clamp=CLAMP[sel], steps=STEPS[sel], n_steps=N_STEPS, stride=STRIDE[sel], height=HEIGHT,
                    limit2=None if limit2 is None else limit2[sel])
        args.update(kw)
        if self.has_tracers:
            args["tracers"] = tracers
        return ens.watch_sweep(**args)

    def watch(self, ens, tracers=False, **kw):
        return ens.watch(tracers=tracers, **kw) if self.has_tracers else ens.watch(**kw)

    def encounters(self, ens, limit2, tracers):
        return ens.encounters(limit2, tracers, True) if self.has_tracers else ens.encounters(limit2, True)

    def targets(self, ens, tracers):
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

    def limit_of(self, k, limits):
        """World k's limit: its own entry, or with limit2=None its own clamp."""
        return CLAMP[k] if limits is None else limits[k]


def _world(got, i):
    rec, rows = got
    return rec[i], {name: rows[name][i] for name in W.ROWS}


@pytest.fixture(params=SHAPES, ids=_id)
def case(request, nb):
    return Case(nb, request.param)


@pytest.fixture(params=ONE_EACH, ids=_id)
def one(request, nb):
    return Case(nb, request.param)


@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_every_world_is_a_one_world_watch_under_its_own_parameters_and_the_state_is_a_sweeps(case, arith):
    c = case
    with c.make(arith=arith) as twin:
        twin.sweep(c.delta, CLAMP, STEPS, n_steps=N_STEPS)
        final = c.state(twin)
        step = (twin.deltas(False) if c.has_tracers else twin.deltas())[1]
    for tracers in c.segments():
        for limits, resume in ((c.limits, False), (None, False), (None, True)):
            with c.make(arith=arith) as ens:
                rec, rows = got = c.wsweep(ens, tracers, limit2=limits, resume=resume)
                assert c.state(ens) == final, f"the rows after watch_sweep(tracers {tracers}) are not those after the sweep"
                assert (ens.deltas(tracers) if c.has_tracers else ens.deltas())[1] == step == N_STEPS
            assert rec.dtype == c.nb.WATCH_DTYPE and rec.shape == (WORLDS,)
            assert [int(r) for r in rec["samples"]] == [len(Q.taken(int(STEPS[k]), int(STRIDE[k]), resume)) for k in c.own]
            assert [int(r) for r in rec["rows"]] == [c.n_targets(k, tracers) for k in c.own] and [int(r) for r in rec["sources"]] == c.sizes
            for k in c.own:
                with c.make([k], arith=arith, clamp=float(CLAMP[k])) as single:
                    want = c.watch(single, tracers, delta=float(c.delta[k]), n_steps=int(STEPS[k]), stride=int(STRIDE[k]), height=HEIGHT,
                                   limit2=None if limits is None else limits[k:k + 1], resume=resume)
                mine, alone = _world(got, k), _world(want, 0)
                assert W.same_world(mine, alone), (f"world {k}, tracers {tracers}, limits {limits is not None}, resume {resume}: "
                                                   f"{W.diff(mine, alone)} differ: got {mine[0]}, expected {alone[0]}")


def _looped(c, ens, limits):
    """What the user's loop sees without watch(): per segment and world the list of (sample, nn_index, nn_d2, targets), one entry
    per state after 0 .. N_STEPS launches of `ens`, which is stepped by sweep(..., n_steps=1): world k moves while s < steps[k]."""
    seen = {tr: [[] for _ in c.own] for tr in c.segments()}
    for s in range(N_STEPS + 1):
        for tr in c.segments():
            _, idx, d2, _ = c.encounters(ens, limits, tr)
            pos = c.targets(ens, tr)
            for i in c.own:
                seen[tr][i].append((s, idx[i], d2[i], pos[i]))
        if s < N_STEPS:
            ens.sweep(c.delta, CLAMP, (STEPS > s).astype(np.int32), n_steps=1)
    return seen


@pytest.mark.parametrize("resume", [False, True])
def test_the_restatement_folds_a_loop_of_single_sweep_steps_into_the_same(one, resume):
    c = one
    limits = c.limits
    with c.make() as twin:
        seen = _looped(c, twin, limits)
    for tracers in c.segments():
        for lim in (limits, None):
            with c.make() as ens:
                got = c.wsweep(ens, tracers, limit2=lim, resume=resume)
            for k in c.own:
                samples = Q.taken(int(STEPS[k]), int(STRIDE[k]), resume)
                want = W.fold([seen[tracers][k][s] for s in samples], c.limit_of(k, lim), HEIGHT, c.n_targets(k, tracers), c.sizes[k], c.dtype)
                mine = _world(got, k)
                assert W.same_world(mine, want), (f"world {k}, tracers {tracers}, samples {samples}: {W.diff(mine, want)} differ: "
                                                  f"got {mine[0]}, expected {want[0]}")


def _raw(c, h, flags, delta, clamp, steps, n_steps, stride, limits, height, out, arrays):
    """nbody_wsweep_<handle> through ctypes: arrays a list of six arrays or None each, or None for rows == NULL."""
    C = c.nb._capi

    def typed(a, ctype):
        return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctype))
    call = getattr(C.load(), "nbody_wsweep_" + c.kind)
    block = None if arrays is None else C.WatchRows(*[None if a is None else a.ctypes.data for a in arrays])
    real = ctypes.c_double if c.dtype == np.float64 else ctypes.c_float
    return call(h.h, flags, typed(delta, real), typed(clamp, ctypes.c_float), typed(steps, ctypes.c_int32), n_steps,
                typed(stride, ctypes.c_int32), typed(limits, ctypes.c_float), height, None if out is None else C._ptr(out),
                None if block is None else ctypes.byref(block), None)


@pytest.mark.parametrize("kind", ["ensemble", "rr"])
def test_a_worlds_outputs_are_the_same_alone_and_whatever_is_asked_for(nb, kind):
    shape = (kind, tuple(Q.RAGGED_N), tuple(Q.RR_M)) if KINDS[kind][2] else (kind, (257,) * WORLDS, (0,) * WORLDS)
    c = Case(nb, shape)
    for tracers in c.segments():
        flags = 1 if tracers else 0
        with c.make() as ens:
            whole = c.wsweep(ens, tracers, limit2=c.limits)
        for k in c.own:                                                 # alone: the same world in a call of one world
            with c.make([k]) as ens:
                alone = c.wsweep(ens, tracers, which=[k], limit2=c.limits)
            assert W.same_world(_world(alone, 0), _world(whole, k)), (k, tracers, W.diff(_world(alone, 0), _world(whole, k)))
        with c.make() as ens:
            rec, none = c.wsweep(ens, tracers, limit2=c.limits, rows=False)
            assert none is None and W.same(rec, whole[0])
        flat = [np.concatenate([np.ravel(a) for a in whole[1][name]]) for name in W.ROWS]
        for mask in (0, 63, 1, 32, 21, 42):                             # which of the six arrays are asked for
            with c.make() as ens:
                out = np.zeros(WORLDS, nb.WATCH_DTYPE)
                arrays = [np.zeros_like(f) if mask >> i & 1 else None for i, f in enumerate(flat)]
                ens.h._check(_raw(c, ens.h, flags, c.delta, CLAMP, STEPS, N_STEPS, STRIDE, c.limits, HEIGHT, out, arrays))
                assert W.same(out, whole[0]), mask
                assert all(a is None or W.same(a, f) for a, f in zip(arrays, flat)), mask


# The split of the contract: every world either runs through the first call on a stride that divides its length, or is finished
# within it.  With the scene's strides [1, 2, 3, 1, 1, 7] and n1 = 6: the worlds 0, 1 and 2 run through (6 is a multiple of 1, 2
# and 3) and take 3, 1 and 3 steps of the second call; the worlds 3, 4 and 5 keep the scene's steps 2, 0 and 5 and are finished.
SPLIT_N1, SPLIT_N2 = 6, 3
SPLIT_STEPS1 = np.array([6, 6, 6, 2, 0, 5], np.int32)
SPLIT_STEPS2 = np.array([3, 1, 3, 0, 0, 0], np.int32)


def test_a_watched_sweep_split_over_two_calls_merges_into_the_whole(one):
    c = one
    assert all((a == SPLIT_N1 and SPLIT_N1 % d == 0) or b == 0 for a, b, d in zip(SPLIT_STEPS1, SPLIT_STEPS2, STRIDE))
    for tracers in c.segments():
        with c.make() as ens:
            whole = c.wsweep(ens, tracers, limit2=c.limits, steps=SPLIT_STEPS1 + SPLIT_STEPS2, n_steps=SPLIT_N1 + SPLIT_N2)
            final = c.state(ens)
        with c.make() as ens:
            first = c.wsweep(ens, tracers, limit2=c.limits, steps=SPLIT_STEPS1, n_steps=SPLIT_N1)
            second = c.wsweep(ens, tracers, limit2=c.limits, steps=SPLIT_STEPS2, n_steps=SPLIT_N2, resume=True)
            assert c.state(ens) == final
        assert list(second[0]["samples"]) == [len(Q.taken(int(s), int(d), True)) for s, d in zip(SPLIT_STEPS2, STRIDE)]
        merged = c.nb.watch_merge(first, second, SPLIT_N1)
        for i in c.own:
            assert W.same_world(_world(merged, i), _world(whole, i)), (i, tracers, W.diff(_world(merged, i), _world(whole, i)))


def test_resume_without_a_step_gives_the_empty_rows_whatever_the_scratch_holds(one):
    c = one
    with c.make() as ens:
        for tracers in c.segments():
            c.wsweep(ens, tracers, limit2=c.limits)                     # leaves other values in the scratch
            before = c.state(ens)
            rec, rows = c.wsweep(ens, tracers, limit2=c.limits, steps=None, n_steps=0, resume=True)
            for k in c.own:
                want = W.fold([], c.limits[k], HEIGHT, c.n_targets(k, tracers), c.sizes[k], c.dtype)
                assert W.same_world(_world((rec, rows), k), want), (k, tracers, W.diff(_world((rec, rows), k), want))
                assert rec["samples"][k] == 0 and rec["isolated_rows"][k] == c.n_targets(k, tracers)
            rec, rows = c.wsweep(ens, tracers, limit2=c.limits, steps=None, n_steps=0)   # and without RESUME: sample 0 in every world
            assert list(rec["samples"]) == [1] * WORLDS
            assert c.state(ens) == before


def _message(err):
    head = f"nbody_hip error {err.code}: "
    assert str(err).startswith(head)
    return str(err)[len(head):]


def test_refusals_name_the_handle_and_wsweep_and_change_nothing(one, nb):
    c = one
    C = nb._capi
    out = np.zeros(WORLDS, nb.WATCH_DTYPE)

    def refused(h, *words, flags=0, delta=c.delta, steps=STEPS, n_steps=N_STEPS, stride=STRIDE, height=0, out_=out):
        with pytest.raises(C.NBodyError) as e:
            h._check(_raw(c, h, flags, delta, CLAMP, steps, n_steps, stride, None, height, out_, None))
        assert e.value.code == C.ERR_INVALID
        msg = _message(e.value)
        assert msg.startswith(c.who + " wsweep: "), msg
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
        refused(ens.h, "delta is NULL", delta=None)
        refused(ens.h, "unknown flag", flags=4)
        refused(ens.h, "unknown flag", flags=0x80000002)
        if not c.has_tracers:
            refused(ens.h, "NBODY_WATCH_TRACERS", "without tracers", flags=C.WATCH_TRACERS)
        refused(ens.h, "n_steps", n_steps=-1)
        refused(ens.h, "steps[0]", "world 0", "n_steps = 3", n_steps=3)
        refused(ens.h, "steps[1]", "world 1", steps=np.array([5, -1, 4, 2, 0, 5], np.int32))
        refused(ens.h, "stride[3]", "world 3", ">= 1", stride=np.array([1, 2, 3, 0, 1, 7], np.int32))
        refused(ens.h, "stride[0]", "world 0", stride=np.array([-2, 2, 3, 0, 1, 7], np.int32))
        refused(ens.h, "height", "2^24", height=(1 << 24) + 1)
        assert not out.view(np.uint8).any()                             # nothing was written
        assert c.state(ens) == before                                   # and nothing stepped
        assert (ens.deltas(False, True) if c.has_tracers else ens.deltas(True))[1] == step
        for tracers in c.segments():                                    # and the handle works
            rec, _ = c.wsweep(ens, tracers, height=1 << 24)
            assert list(rec["samples"]) == [len(Q.taken(int(s), int(d))) for s, d in zip(STEPS, STRIDE)]
