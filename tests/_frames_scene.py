"""The scene of the ensemble-frames tests (test_gpu_ensemble_frames.py; test_ensemble_frames_host.py checks on the CPU that the
oracle's draw() treats every planted row as this file says).  Pure numpy, no GPU.

A world is `n` body rows and `m` tracer rows.  All worlds of a scene share one list of POSITIONS (a world takes a prefix of it),
but every world has velocities and weights of its own: a row that leaks into another world's tile changes bytes there.

Lengths are fractions of `height`; "pixel (r, c)" means row r, column c at render_px = 100 (a cell is height / 100).  Random rows
are spread over [-0.05, 1.05)^2 of the height, so some fall outside, and are kept out of pixel rows 40 and 41, which belong to
the planted rows (bodies first in the list, `N_PLANTED` of them; a world with fewer bodies takes random rows only):

  (40, 10) (40, 12) (40, 14)   exactly 24, 25 and 26 light rows: alpha 240, 250, 250
  (40, 20)                     a heavy row BEFORE three light ones: green
  (40, 22)                     three light rows and a heavy one AFTER them: green
  (40, 30) (40, 31)            weight 10 (light) and weight 11 (heavy)
  (40, 35)                     two light rows, the later with the SMALLER v: the later one colours the pixel (a max over v is wrong)
  (40, 40)                     one light body; planted tracer 0 sits on it and colours it (tracers are the last rows)
  (40, 42)                     one heavy body; planted tracer 1 sits on it and the pixel stays green
  (40, 50) .. (40, 54)         light rows with velocities (inf, 0), (NaN, 1), (25, 0.5): 255 as u8, (25, 0.4): 254, (23.5, 0.35): 238
  positions (NaN, .5), (.5, NaN): nowhere;  (-0, -0): pixel (0, 0);  (1, .5) and (.5, 1) of the height exactly: outside;
  (nextafter(height, 0),) * 2: pixel (99, 99)
Planted tracers (`M_PLANTED`, for a world with at least that many): the two above, one at a NaN position, one at (40, 44) with
velocity (-inf, NaN), one outside at exactly the height."""
import numpy as np

BAND = (0.40, 0.42)      # pixel rows 40 and 41 at render_px = 100
ROW = 40


def _planted_bodies(h, dtype):
    """-> (pos[P,2], vel[P,2] or NaN where the world's own velocity is kept, weight[P] or 0 where the world's own light weight is)."""
    u = h / 100.0
    at = lambda c, r=ROW: ((c + 0.5) * u, (r + 0.5) * u)  # noqa: E731  (x, y) of pixel (r, c)
    keep = (np.nan, np.nan)
    rows = []     # (pos, vel, weight); weight 0: a light weight of the world's own

    def add(p, v=keep, w=0):
        rows.append((p, v, w))

    for c, k in ((10, 24), (12, 25), (14, 26)):
        for _ in range(k):
            add(at(c))
    add(at(20), w=11)
    for _ in range(3):
        add(at(20))
    for _ in range(3):
        add(at(22))
    add(at(22), w=4_000_000_000)
    add(at(30), w=10)
    add(at(31), w=11)
    add(at(35), v=(-12.0, 8.0))      # v = 0x10 + 200
    add(at(35), v=(0.5, -0.5))       # v = 0x10 + 10: the later row, the smaller v
    add(at(40))
    add(at(42), w=12)
    add(at(50), v=(np.inf, 0.0))
    add(at(51), v=(np.nan, 1.0))
    add(at(52), v=(-25.0, 0.5))
    add(at(53), v=(25.0, -0.4))
    add(at(54), v=(23.5, 0.35))
    add((np.nan, 0.5 * h))
    add((0.5 * h, np.nan))
    add((-0.0, -0.0))
    add((h, 0.5 * h))
    add((0.5 * h, h))
    top = float(np.nextafter(dtype(h), dtype(0)))
    add((top, top))
    pos = np.array([r[0] for r in rows], dtype)
    vel = np.array([r[1] for r in rows], dtype)
    w = np.array([r[2] for r in rows], np.uint32)
    return pos, vel, w


def _planted_tracers(h, dtype):
    u = h / 100.0
    pos = np.array([((40 + 0.5) * u, (ROW + 0.5) * u), ((42 + 0.5) * u, (ROW + 0.5) * u), (np.nan, np.nan),
                    ((44 + 0.5) * u, (ROW + 0.5) * u), (h, h)], dtype)
    vel = np.array([(3.0, -4.0), (1.0, 1.0), (1.0, 1.0), (-np.inf, np.nan), (0.0, 0.0)], dtype)
    return pos, vel


N_PLANTED = len(_planted_bodies(100.0, np.float32)[0])
M_PLANTED = len(_planted_tracers(100.0, np.float32)[0])


def _spread(rng, count, h, dtype):
    """Random positions over [-0.05 h, 1.05 h)^2, none in the planted band."""
    pos = (rng.uniform(-0.05, 1.05, (count, 2)) * h).astype(dtype)
    lo, hi = dtype(BAND[0] * h), dtype(BAND[1] * h)
    y = pos[:, 1]
    y[(y >= lo) & (y < hi)] += dtype(0.02 * h)
    return pos


def scene(sizes, counts, dtype, height=100_000, seed=7):
    """-> one dict per world: pos[n,2], vel[n,2], w[n] (uint32), tpos[m,2], tvel[m,2] (m may be 0), all of `dtype`."""
    dtype = np.dtype(dtype).type
    h = float(height)
    rng = np.random.default_rng(seed)
    n_max, m_max = max(sizes), max(max(counts), 1)
    pp, pv, pw = _planted_bodies(h, dtype)
    tp_, tv_ = _planted_tracers(h, dtype)
    rand_pos = _spread(rng, n_max, h, dtype)
    rand_tpos = _spread(rng, m_max, h, dtype)
    worlds = []
    for k, (n, m) in enumerate(zip(sizes, counts)):
        wr = np.random.default_rng(seed * 1000 + k)
        vel_own = (wr.standard_normal((n_max + N_PLANTED, 2)) * (2.0 + 3.0 * k)).astype(dtype)   # |vx|+|vy| on both sides of 23.9
        w_own = wr.integers(1, 21, n_max + N_PLANTED).astype(np.uint32)                           # about half of them heavy
        tvel_own = (wr.standard_normal((m_max + M_PLANTED, 2)) * (2.0 + 3.0 * k)).astype(dtype)
        if n >= N_PLANTED:
            pos = np.concatenate([pp, rand_pos[:n - N_PLANTED]])
            vel = vel_own[:n].copy()
            own = np.isnan(pv).all(axis=1)
            vel[:N_PLANTED][~own] = pv[~own]
            w = w_own[:n].copy()
            w[:N_PLANTED] = np.where(pw == 0, 1 + w_own[:N_PLANTED] % 10, pw)                    # the world's own LIGHT weight: 1 .. 10
        else:
            pos, vel, w = rand_pos[:n].copy(), vel_own[:n].copy(), w_own[:n].copy()
        if m >= M_PLANTED:
            tpos = np.concatenate([tp_, rand_tpos[:m - M_PLANTED]])
            tvel = np.concatenate([tv_, tvel_own[:m - M_PLANTED]])
        else:
            tpos, tvel = rand_tpos[:m].copy(), tvel_own[:m].copy()
        worlds.append(dict(pos=np.ascontiguousarray(pos, dtype), vel=np.ascontiguousarray(vel, dtype), w=w,
                           tpos=np.ascontiguousarray(tpos, dtype).reshape(-1, 2), tvel=np.ascontiguousarray(tvel, dtype).reshape(-1, 2)))
    return worlds


def draw_world(orc, world, height, render_px, tracers, state=None):
    """The yardstick: the oracle's draw() of the world's own rows — its bodies, then (tracers=True) its tracers as rows of
    weight 1.  state: (pos, vel, tpos, tvel) to draw in place of the scene's own."""
    pos, vel, tpos, tvel = state if state is not None else (world["pos"], world["vel"], world["tpos"], world["tvel"])
    w = world["w"]
    if tracers and len(tpos):
        pos, vel = np.concatenate([pos, tpos]), np.concatenate([vel, tvel])
        w = np.concatenate([w, np.ones(len(tpos), np.uint32)])
    return orc.draw(pos, vel, w, height, render_px)
