"""Ensembles: many small worlds of one size, stepped together (nbody_ensemble_*, include/nbody_hip.h).

The same scene under many seeds, a sweep over initial conditions, many independent clusters: below a few thousand bodies one
world cannot fill the device, and one `World` per world costs one launch chain per world and step.  An `Ensemble` holds B worlds
of n bodies each (n <= 4096) on the device and steps all of them with one launch per step; every world takes the step of
`World(method="direct")`, independently of the others — EXACT bit-identical to the oracle's update_direct of that world alone,
FAST within the tolerance of DESIGN.md, AUTO choosing between them per world and per step on the device.

Everything is float32.  Shapes, dtypes and the size limits are checked here, with ValueError, before a handle exists.
"""
from __future__ import annotations

import numpy as np

from . import _capi
from ._capi import Counting

MAX_BODIES = 4096          # per world: its sources stage whole in LDS
MAX_ROWS = 1 << 26         # worlds * bodies

_ARITH = {"auto": _capi.ARITH_AUTO, "fast": _capi.ARITH_FAST, "exact": _capi.ARITH_EXACT}


def _checked(position, velocity, weight):
    """-> (B, n, position[B,n,2], velocity[B,n,2], weight[B,n] or None), contiguous; ValueError for anything else."""
    position, velocity = np.asarray(position), np.asarray(velocity)
    for name, a in (("position", position), ("velocity", velocity)):
        if a.dtype != np.float32:
            raise ValueError(f"Ensemble: {name} must be float32 (got {a.dtype}); ensembles are f32 only")
    if position.ndim == 2:   # one world
        position = position[None]
        if velocity.ndim == 2:
            velocity = velocity[None]
        if weight is not None and np.ndim(weight) == 1:
            weight = np.asarray(weight)[None]
    if position.ndim != 3 or position.shape[2] != 2:
        raise ValueError(f"Ensemble: position must be [B, n, 2] (or [n, 2] for one world), got {position.shape}")
    if velocity.shape != position.shape:
        raise ValueError(f"Ensemble: velocity {velocity.shape} does not match position {position.shape}")
    b, n = position.shape[:2]
    if b < 1:
        raise ValueError("Ensemble: at least one world")
    if not 1 <= n <= MAX_BODIES:
        raise ValueError(f"Ensemble: 1 .. {MAX_BODIES} bodies per world, got {n} (above that a World per world is the tool)")
    if b * n > MAX_ROWS:
        raise ValueError(f"Ensemble: worlds * bodies = {b * n} exceeds 2^26")
    if weight is not None:
        weight = np.asarray(weight)
        if weight.shape != (b, n):
            raise ValueError(f"Ensemble: weight must be [B, n] = {(b, n)}, got {weight.shape}")
        if weight.dtype.kind not in "ui":
            raise ValueError(f"Ensemble: weight must be an integer array (u32 upstream), got {weight.dtype}")
        weight = np.ascontiguousarray(weight, dtype=np.uint32)
    return b, n, np.ascontiguousarray(position), np.ascontiguousarray(velocity), weight


class Ensemble:
    def __init__(self, position, velocity, weight=None, *, device=0, clamp=0.001, arith="auto"):
        """position, velocity [B, n, 2] float32 (2-D: one world), weight [B, n] integers or None (all 1)."""
        if arith not in _ARITH:
            raise ValueError(f"arith must be one of {sorted(_ARITH)}")
        self.h = None
        args = _checked(position, velocity, weight)
        self.h = _capi.EnsembleHandle(device)
        self.h.set_params(clamp=float(clamp), arith=_ARITH[arith])
        self._upload(*args)

    def _upload(self, b, n, position, velocity, weight):
        self.h.upload(b, n, position, velocity, weight)
        self._weight = np.ones((b, n), np.uint32) if weight is None else weight.copy()

    def upload(self, position, velocity, weight=None):
        """Replaces the ensemble by another one, of any shape."""
        self._upload(*_checked(position, velocity, weight))

    @property
    def shape(self):
        """(worlds, bodies per world)."""
        return self.h.shape

    def update(self, delta: float, counter: Counting | None = None, n_steps: int = 1):
        """n_steps direct steps of every world (World::update, main.rs:388-425, with the direct sum as its force phase); the
        call's seconds go to counter.sum_gravity."""
        self.h.update(delta, n_steps, counter)

    def particles(self):
        """-> (position[B,n,2], velocity[B,n,2], weight[B,n]); rows never move."""
        pos, vel = self.h.download()
        return pos, vel, self._weight.copy()

    def accel(self):
        """-> acc[B,n,2]: the accelerations at the current positions; the state is untouched."""
        return self.h.accel()

    def close(self):
        if getattr(self, "h", None) is not None:
            self.h.close()
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
