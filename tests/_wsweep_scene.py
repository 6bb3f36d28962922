"""What the watched sweep's host and device tests share (tests/test_ensemble_wsweep_host.py, tests/test_gpu_ensemble_wsweep.py):
the sample rule in three lines, the six worlds' parameters, and the scene — the encounters' worlds (tests/_encounters_scene.py)
under the watch tests' velocities.

Parameters.  Six worlds, n_steps = 5.  The deltas are pairwise distinct; neighbouring worlds have different clamps, 0.3 and 1.5,
and the handle's own params.clamp is a third value, 0.25, so that "limit2=None means clamp[k]" differs from "means params.clamp"
wherever a pair lies between: the lattice worlds (k % 3 == 1) keep their neighbours at d2 = 1 — the planted pair, which the host
test shows to stay between 0.3 and 1.5 over the run.  steps = [5, 1, 4, 2, 0, 5], stride = [1, 2, 3, 1, 1, 7]: world 4 never
steps, world 5's stride exceeds its steps (sample 0 alone, and none under RESUME), world 1 is finished before its stride comes
round again, and under RESUME the worlds' first samples are 1, none, 3, 1, none, none — three different answers in one call."""
import numpy as np

import _encounters_scene as S

F32, F64 = np.float32, np.float64
WORLDS = 6
N_STEPS = 5
STEPS = np.array([5, 1, 4, 2, 0, 5], np.int32)
STRIDE = np.array([1, 2, 3, 1, 1, 7], np.int32)
DT = 2.0 ** -10
DELTA = DT * np.array([1.0, 2.0, 0.5, 3.0, 1.5, 0.75])
CLAMP = np.array([0.3, 1.5, 0.3, 1.5, 0.3, 1.5], np.float32)
PARAM_CLAMP = 0.25                                  # the handles' own clamp: no world's
HEIGHT = 8
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


def takes(s, steps, stride, resume=False):
    """The rule of include/nbody_ensemble.h ("a watched sweep", Samples), word for word."""
    return s <= steps and s % stride == 0 and not (s == 0 and resume)


def taken(steps, stride, resume=False, n_steps=None):
    """The sample numbers a world takes in a call of n_steps steps (None: its own steps)."""
    return [s for s in range((steps if n_steps is None else n_steps) + 1) if takes(s, steps, stride, resume)]


def scene(kind, sizes, counts):
    """-> (list of worlds: dicts of pos, vel, tpos, tvel in the kind's dtype, limits float32[worlds])."""
    dtype = KINDS[kind][1]
    seed = S.seed_of("wsweep", kind, tuple(sizes), tuple(counts))
    worlds = []
    for k, (n, m) in enumerate(zip(sizes, counts)):
        pos = S.world(seed, k, n, dtype)
        rng = np.random.default_rng([seed, k, 99])
        worlds.append(dict(pos=pos, vel=rng.uniform(-1, 1, (n, 2)).astype(dtype), tpos=S.tracers(seed, k, m, dtype, pos),
                           tvel=rng.uniform(-1, 1, (m, 2)).astype(dtype)))
    return worlds, S.limits(len(sizes), shift=sizes[0] + counts[-1])


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
