"""The scene of the ensemble-summary tests (test_ensemble_summary_host.py, test_gpu_ensemble_summary.py).  Pure numpy, no GPU.

Benign data cannot see the order of a sum: with positions in [0, 1e5) and small weights every weighted sum is exact in double and
any order gives the same bits.  So every coordinate here is +-2^u (1 + v), u uniform in [-30, 40], v uniform in [0, 1), and every
velocity the same draw scaled by 2^-20: the terms of a sum span 70 binades and a different order rounds differently
(test_ensemble_summary_host.py asserts that on these very rows).

A world's rows depend on (seed, world index k, its number of rows, dtype) only, so a world is the same rows whatever ensemble
it is put into.  A segment of at least MIN_PLANTED rows has these rows planted at slots of its own (`planted(...)` names them):
  nan_x, nan_y, nan_vx, nan_vy, pinf_*, ninf_*   one component NaN / +inf / -inf, the other three finite: not counted
  inside_nan_v     position (H/2, H/3), velocity (NaN, 1): in bounds, not counted
  edge_out         position (H, 1): outside by position (x < H fails); finite: counted     (not in a "zeros" world, below)
  edge_in          position (nextafter(H, 0), 0): inside                                    (not in a "zeros" world)
  w10, w11, w2p24, wmax   (bodies) weights 10, 11, 2^24 + 1 (rounds to 2^24 as f32) and 2^32 - 1 (rounds to 2^32 as f32)
World kinds, by k % 4 (segments of at least MIN_PLANTED rows):
  1   "zeros": every x is made <= -0.0 and every y >= +0.0, and two planted rows hold (-0.0, +0.0) and (+0.0, -0.0): max_x is
      +0.0 and min_y is -0.0 — the zeros are the extreme values and their signs decide
  2   float64 only, "huge": one planted row has velocity (1e200, -1e200): its squared speed, max_speed2 and sum_wv2 are +inf
H = HEIGHT = 100 000."""
import numpy as np

HEIGHT = 100_000
MIN_PLANTED = 32
SEED = 20261021

_NAMES = ([f"{s}_{c}" for s in ("nan", "pinf", "ninf") for c in ("x", "y", "vx", "vy")] +
          ["inside_nan_v", "edge_out", "edge_in", "zero_a", "zero_b", "huge_v", "w10", "w11", "w2p24", "wmax"])


# The seed of the segments of n rows where one was searched for (test_ensemble_summary_host.py, "visibility": with it every
# rival order gives other bits than the contract's in all six ordered sums of world 0, measured from world 1); SEED elsewhere.
SEEDS = {  # (rows, bytes of an element, tracers): seed
    (600, 4, False): 20266982,
    (4096, 4, False): 20261031,
    (4097, 4, True): 20261069,
    (9000, 4, True): 20292433,
    (600, 8, False): 20261738,
    (4096, 8, False): 20261054,
    (4097, 8, True): 20261027,
    (9000, 8, True): 20268030,
}


def seed_of(n, dtype, tracers=False):
    return SEEDS.get((int(n), np.dtype(dtype).itemsize, bool(tracers)), SEED)


def _draw(rng, shape, dtype, scale=0):
    u = rng.uniform(-30.0, 40.0, shape)
    v = rng.uniform(0.0, 1.0, shape)
    sign = np.where(rng.integers(0, 2, shape) == 0, 1.0, -1.0)
    return (sign * np.exp2(u + scale) * (1.0 + v)).astype(dtype)


def _rng(seed, k, n, dtype, tracers):
    return np.random.default_rng([seed, k, n, np.dtype(dtype).itemsize, int(tracers)])


def planted(seed, k, n, dtype, tracers=False):
    """-> {name: row} of the planted rows of this segment ({} below MIN_PLANTED rows)."""
    if n < MIN_PLANTED:
        return {}
    slots = _rng(seed + 1, k, n, dtype, tracers).permutation(n)[:len(_NAMES)]
    return {name: int(s) for name, s in zip(_NAMES, slots)}


def segment(seed, k, n, dtype, tracers=False):
    """-> (pos[n,2], vel[n,2], weight uint32[n]) of world k's bodies (tracers=True: its tracers, every weight 1)."""
    dtype = np.dtype(dtype).type
    rng = _rng(seed, k, n, dtype, tracers)
    pos = _draw(rng, (n, 2), dtype)
    vel = _draw(rng, (n, 2), dtype, scale=-20)
    w = np.ones(n, np.uint32) if tracers else rng.integers(1, 21, n).astype(np.uint32)
    at = planted(seed, k, n, dtype, tracers)
    if not at:
        return pos, vel, w
    if k % 4 == 1:
        pos[:, 0] = -np.abs(pos[:, 0])
        pos[:, 1] = np.abs(pos[:, 1])
        pos[at["zero_a"]] = (-0.0, 0.0)
        pos[at["zero_b"]] = (0.0, -0.0)
    if k % 4 == 2 and dtype is np.float64:
        vel[at["huge_v"]] = (1e200, -1e200)
    for s, value in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf)):
        for c, (arr, col) in (("x", (pos, 0)), ("y", (pos, 1)), ("vx", (vel, 0)), ("vy", (vel, 1))):
            arr[at[f"{s}_{c}"], col] = value
    h = dtype(HEIGHT)
    pos[at["inside_nan_v"]] = (h / 2, h / 3)
    vel[at["inside_nan_v"]] = (np.nan, 1.0)
    if k % 4 != 1:  # (a "zeros" world keeps every finite x at or below zero)
        pos[at["edge_out"]] = (h, 1.0)
        pos[at["edge_in"]] = (np.nextafter(h, dtype(0)), 0.0)
    if not tracers:
        for name, value in (("w10", 10), ("w11", 11), ("w2p24", (1 << 24) + 1), ("wmax", (1 << 32) - 1)):
            w[at[name]] = value
    return pos, vel, w


def scene(sizes, counts, dtype):
    """-> one dict per world: pos[n,2], vel[n,2], w[n] (uint32), tpos[m,2], tvel[m,2] (m may be 0), all of `dtype`."""
    worlds = []
    for k, (n, m) in enumerate(zip(sizes, counts)):
        pos, vel, w = segment(seed_of(n, dtype), k, n, dtype)
        tpos, tvel, _ = segment(seed_of(m, dtype, True), k, m, dtype, tracers=True)
        worlds.append(dict(pos=pos, vel=vel, w=w, tpos=tpos, tvel=tvel))
    return worlds
