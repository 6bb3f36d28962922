"""Which walk ran: a parser for the `walk route:` lines of NBODY_TRACE=1 (tree_driver.hip, trace_route), and the rule by which
tree_walk_phase chooses, restated.

Nearly every route of a Barnes-Hut step computes the same bits by design, so a comparison with the oracle passes whichever
ran.  A test that names a route asserts it from these lines (read with `capfd`).
"""
import re
from collections import namedtuple

Route = namedtuple("Route", "route arm rows srec rec_mode prep ahead n_tgt f64")
_LINE = re.compile(r"^\[nbody\] walk route: route=(\S+) arm=(\S+) rows=(-?\d+) srec=(-?\d+) rec_mode=(-?\d+) prep=(\S+) ahead=([01]) "
                   r"n_tgt=(\d+) f64=([01])$", re.M)

FUSED, SMALL, PER_THREAD, TILE, THREE_PASS = "fused", "small-leaves", "per-thread", "tile", "three-pass"
TILE_MIN_TARGETS = 4096       # mode 1 takes the one-pass walk from here on (tree_walk_phase)
BIG_LEAF = 16                 # leaves of at least this many bodies are "big" (driver.h, walk_args)


def parse(err):
    """Every route line of a captured stderr, in order."""
    return [Route(m[1], m[2], int(m[3]), int(m[4]), int(m[5]), m[6], int(m[7]), int(m[8]), int(m[9])) for m in _LINE.finditer(err)]


def routes(err, ahead=None):
    """The set of route names that ran (ahead: only the walks of steps enqueued ahead / only the others)."""
    return {r.route for r in parse(err) if ahead is None or r.ahead == int(ahead)}


def kernels(err, route=TILE):
    """The distinct kernel instantiations of one route: (arm, rows, srec, rec_mode)."""
    return {(r.arm, r.rows, r.srec, r.rec_mode) for r in parse(err) if r.route == route}


def expected_bvh_route(n, leaf, mode, lab, fast=False):
    """tree_walk_phase's rule for a BVH walk over the n bodies themselves, without statistics, first walks of a context (no
    back-off yet): big leaves are leaves >= 16; mode 3 (one pass) and mode 2 (three passes, laboratory library only: the
    product reads 2 and 4 as 1) are forced; mode 1 needs n >= 4096, and so does 4."""
    mode = int(mode)
    if not lab and mode in (2, 4):
        mode = 1
    if leaf < BIG_LEAF:
        return FUSED if fast else SMALL
    if mode == 3 or (mode == 1 and n >= TILE_MIN_TARGETS):
        return TILE
    if mode == 2 or (mode == 4 and n >= TILE_MIN_TARGETS):
        return THREE_PASS
    return FUSED


def expected_tile_kernel(f64, fast, rows=8, srec=1, fast_rows=-1, rec_mode=3, wave_log=0, bfs=0):
    """choose_tile_route's rule (csrc/walk_route.h) for the one-pass walk's kernel, as kernels() reports it: (arm, rows, srec,
    rec_mode).  The defaults are the product's knobs; the laboratory library reads NBODY_WALK_TILE_TARGETS, _SCALAR_REC,
    _FAST_ROWS, _FAST_REC, _WAVE_LOG and _FAST_BFS into them.  Exact walks take the LDS rows; FAST takes them in f64 or where
    fast_rows says so, else the registers (breadth first: f32 only, never with the log; the log has one kernel, record mode 0)."""
    rows = rows if rows in (4, 16) else 8
    through_rows = bool(fast_rows) if fast_rows >= 0 else bool(f64)
    if not fast or through_rows:
        return ("fast-rows" if fast else "exact", rows, 1 if srec else 0, -1)
    if wave_log:
        return ("fast-registers-log", -1, -1, 0)
    if bfs and not f64:
        return ("fast-bfs", -1, -1, -1)
    return ("fast-registers", -1, -1, rec_mode if rec_mode in (1, 3) else 0)
