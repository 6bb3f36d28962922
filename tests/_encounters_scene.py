"""The scene of the encounters' tests (tests/test_ensemble_encounters_host.py, tests/test_gpu_ensemble_encounters.py): worlds of
any size and dtype from a seed, three kinds by k % 3, and the plants the contract's edges need.

kind 0, "plain".  Rows spread over 16 binades with both signs, so a fused d2 rounds differently somewhere.  From 16 rows on it
    holds the plants of `planted`: a pair whose difference is subnormal (skipped), a pair with a normal dx whose d2 underflows to
    +0 (live, close, the world's minimum), two coincident bodies beside a third, and rows holding NaN, +inf, -inf and -0.0.  The
    two bodies of each pair sit at opposite ends of the world, so from 257 rows on they are in different target tiles and from
    1025 on in different source chunks.
kind 1, "lattice".  The integer points of a square: every d2 is an exact small integer and most rows have two to four nearest
    neighbours at d2 == 1, so another tie rule gives other indices (and a fused d2 gives the same bits: nothing is rounded).
kind 2, "edge".  One body: no pair at all.  Two bodies: 2^127 apart (2^1023 in float64), so `sum` is finite and d2 overflows to
    +inf: a live pair.  More: a plain world from another seed, without plants, shifted away from the origin.

Tracers: kind 0 and 2 spread as the bodies are, and from 8 on three plants (`planted_tracers`): one on top of a body (a skipped
pair), one at NaN (isolated) and one far outside.  Kind 1: the centres of the lattice's cells, four bodies at the same d2."""
import zlib

import numpy as np

LIMITS = (1.5, float("nan"), 0.0, float("inf"), 0.3)       # world k of a call gets LIMITS[(k + shift) % 5]
#   1.5 lies between the lattice's d2 = 1 and 2 (and between the coincident pair's neighbour at 0.25 and the rest); 0.3 just
#   above that 0.25; NaN and 0 make nothing close, +inf everything with a finite d2.


def seed_of(*what):
    return zlib.crc32(repr(what).encode())


def limits(n_worlds, shift=0):
    return np.array([LIMITS[(k + shift) % len(LIMITS)] for k in range(n_worlds)], np.float32)


def _spread(rng, n, dtype):
    mag = np.exp2(rng.uniform(-6.0, 10.0, (n, 2))) * rng.uniform(1.0, 2.0, (n, 2))
    return (mag * rng.choice([-1.0, 1.0], (n, 2))).astype(dtype)


def planted(n, dtype):
    """name -> row of kind 0's plants in a world of n >= 16 rows."""
    return {"sub_a": 0, "sub_b": n - 1, "under_a": 1, "under_b": n - 2, "coin_a": 2, "coin_b": n - 3, "coin_third": 3,
            "nan": n // 2, "pinf": 4, "ninf": n - 4}


def planted_tracers(m):
    return {"on_body": 0, "nan": m // 2, "far": m - 1}


def tiny_normal_step(dtype):
    """A difference that is a normal number whose square underflows to +0."""
    return dtype(2.0 ** -100) if dtype == np.float32 else dtype(2.0 ** -600)


def world(seed, k, n, dtype):
    """World k's bodies: [n, 2] of dtype."""
    dtype = np.dtype(dtype).type
    rng = np.random.default_rng([seed, k, n])
    kind = k % 3
    if kind == 1:
        side = int(np.ceil(np.sqrt(max(n, 1))))
        i = np.arange(n)
        return np.stack([i % side, i // side], axis=1).astype(dtype)
    if kind == 2:
        if n == 1:
            return np.array([[3.0, -0.0]], dtype)
        if n == 2:
            big = dtype(2.0 ** 126) if dtype == np.float32 else dtype(2.0 ** 1022)
            return np.array([[-big, 0.0], [big, 0.0]], dtype)
        return _spread(rng, n, dtype) + dtype(4096.0)
    pos = _spread(rng, n, dtype)
    if n >= 16:
        at = planted(n, dtype)
        step = tiny_normal_step(dtype)
        pos[at["sub_a"]] = (-0.0, 0.0)
        pos[at["sub_b"]] = (3 * np.finfo(dtype).smallest_subnormal, 0.0)
        pos[at["under_a"]] = (step, 8.0)
        pos[at["under_b"]] = (2 * step, 8.0)
        pos[at["coin_a"]] = pos[at["coin_b"]] = (100000.5, 200000.25)
        pos[at["coin_third"]] = (100000.5, 200000.75)
        pos[at["nan"]] = (np.nan, 3.0)
        pos[at["pinf"]] = (np.inf, 1.0)
        pos[at["ninf"]] = (2.0, -np.inf)
    return pos


def tracers(seed, k, m, dtype, bodies):
    """World k's tracers: [m, 2] of dtype, around `bodies`."""
    dtype = np.dtype(dtype).type
    rng = np.random.default_rng([seed, k, m, 7])
    if k % 3 == 1:
        side = int(np.ceil(np.sqrt(max(bodies.shape[0], 1))))
        i = np.arange(m) % max(bodies.shape[0], 1)
        return (np.stack([i % side, i // side], axis=1) + 0.5).astype(dtype)
    pos = _spread(rng, m, dtype)
    if k % 3 == 2 and bodies.shape[0] > 2:
        pos = pos + dtype(4096.0)
    if m >= 8:
        at = planted_tracers(m)
        if bodies.shape[0]:
            pos[at["on_body"]] = bodies[bodies.shape[0] // 3]
        pos[at["nan"]] = (1.0, np.nan)
        pos[at["far"]] = (-3.0e7, 5.0e7)
    return pos
