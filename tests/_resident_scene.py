"""Scenes and comparisons of the resident-run tests (tests/test_gpu_ensemble_resident.py): the worlds of the sweep tests, restated.

Bodies in the box [1, 5)^2 (inside FAST's domain in both precisions), integer masses 1 .. 11, and in every world of two or more
bodies a planted pair 2^-10 apart: d^2 = 9.5e-7 is below every clamp used here, so the pair's term is another number under each of
them.  Six worlds, pairwise distinct deltas, neighbouring worlds with different clamps — one of them, 1e-6, below kFastClampFloor
= 2^-19, so that world is EXACT under every arith — and step counts from 0 to n_steps = 4."""
import functools

import numpy as np

NTH = 16
B = 6
DELTA = np.array([0.13, 0.4, 0.1, 0.2, 0.05, 0.07])
CLAMP = np.array([1e-3, 1e-2, 1e-6, 1e-3, 1e-2, 2.5e-4], np.float32)
STEPS = np.array([3, 1, 4, 2, 0, 4], np.int32)          # of n_steps = 4
STILL = 4                                                # the world of 0 steps
FLOOR = np.float32(1.9073486328125e-06)                  # kFastClampFloor, 2^-19
PAIR = 2.0 ** -10

assert len(set(DELTA)) == B and all(CLAMP[k] != CLAMP[(k + 1) % B] for k in range(B)) and (CLAMP < FLOOR).sum() == 1
assert STEPS[STILL] == 0 and STEPS.max() == 4


def word(dtype):
    """The unsigned word as wide as an element of `dtype` (4 or 8 bytes)."""
    return {4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_same(got, want, what):
    """Bit for bit, counted in words of the arrays' width."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    w = word(got.dtype)
    diff = int((got.view(w) != want.view(w)).sum())
    assert diff == 0, f"{what}: {diff} of {got.size} words differ"


def world(n, seed, dtype):
    """One world of n bodies -> (pos[n, 2], vel[n, 2], w[n])."""
    dtype = np.dtype(dtype).type
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 2)) * 4 + 1).astype(dtype)
    if n >= 2:
        pos[1] = pos[0] + np.array([PAIR, 0], dtype)
    vel = (rng.standard_normal((n, 2)) * 0.1).astype(dtype)
    w = ((np.arange(n) * (seed % 7 + 3)) % 11 + 1).astype(np.uint32)
    return pos, vel, w


def specials(dtype):
    """-0.0, an infinity and a NaN with a payload: bits no arithmetic hands back."""
    if np.dtype(dtype) == np.float32:
        nan = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    else:
        nan = np.array([0x7FF8000000012345], np.uint64).view(np.float64)[0]
    return np.array([-0.0, nan, np.inf], dtype=dtype)


@functools.lru_cache(maxsize=None)
def scene(n, dtype_name, worlds=B, still=True):
    """`worlds` worlds of n bodies -> (pos[B, n, 2], vel[B, n, 2], w[B, n]), read-only and shared between the tests.  With
    `still` the velocities of world STILL begin with the special values (as many as its 2 n numbers hold)."""
    parts = [world(n, 7000 + 13 * n + k, dtype_name) for k in range(worlds)]
    out = tuple(np.stack([p[i] for p in parts]) for i in range(3))
    if still and worlds > STILL:
        sp = specials(dtype_name)[:2 * n]
        out[1][STILL].reshape(-1)[:len(sp)] = sp
    for a in out:
        a.setflags(write=False)
    return out


def outside_fast(x):
    """fast_domain.h's outside_fast in numpy, in the array's own precision: not finite, at or above 2^60 (f64: 2^100) in
    magnitude, or non-zero and below 2^-22 (f64: 2^-300)."""
    x = np.asarray(x)
    big, tiny = (2.0 ** 60, 2.0 ** -22) if x.dtype == np.float32 else (2.0 ** 100, 2.0 ** -300)
    a = np.abs(x)
    with np.errstate(invalid="ignore"):
        return ~(a < x.dtype.type(big)) | ((a != 0) & (a < x.dtype.type(tiny)))


def cls_of(nb, dtype_name, kind="Ensemble"):
    return getattr(nb, kind + ("64" if np.dtype(dtype_name) == np.float64 else ""))
