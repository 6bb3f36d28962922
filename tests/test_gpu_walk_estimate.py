"""The one-pass walk's preparation alone — the estimate's scan by its three routes, the budget, and the verdict on a
speculated build — against plain integer arithmetic (numpy on uint64, Python ints).  Needs an MI355X.

nbody_selftest_walk_estimate runs launch_tree_walk_tile_prep and nothing else: no walk kernel, no tree.  Routes: 0 the
library scan + walk_check_wrap_est + walk_tile_total (a plain step); 1 the library scan + walk_check_est_tail (a step enqueued
ahead above 2^24 bodies); 2 walk_scan_est_tail, the single-pass scan with decoupled look-back (every other step enqueued
ahead).  Everything here is exact: integers."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
U32, U64 = np.uint32, np.uint64
LIMIT = 2 ** 31 - 1            # the largest total the budget arithmetic takes (31 bits)
K_TILE_BUDGET = 8192           # walk_device.h, kTileBudget
ROUTES = (0, 1, 2)
ACCEPT = dict(nodes=5, node_count=7, fallback=0, bad_index=0, long_nodes=0, level_end=3, node_cap=10)

SIZES = [1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65 * 1024, 65 * 1024 + 1, 66 * 1024 + 1, 130 * 1024 + 3, 2 ** 20 + 1]


# ---- the rules, restated
def extra_waves(n):
    """launch_tree_walk_tile_prep: the waves the walk aims at beyond the head count (tile_waves_target), at least 256."""
    return max(max(n // 64 + 1024, 6656) - n // 64, 256)


def budget_of(total, extra, shift):
    """tile_budget: kTileBudget scaled like the estimate, floor 64, ceil(total / extra), cap 2^30."""
    return min(max(K_TILE_BUDGET >> shift, 64, -(-total // extra)), 2 ** 30)


def groups_of(route, n):
    """Work-groups of the kernel that ends the preparation: none that counts itself (route 0), clamp(n / 2048, 32, 128)
    (walk_check_est_tail), one per 1 024 targets (walk_scan_est_tail)."""
    return [0, min(max(n // 2048, 32), 128), (n + 1023) // 1024][route]


def reference(hist, ids, shift):
    e = hist[ids].astype(U64) >> U64(shift)
    off = np.zeros(e.size, U64)
    np.cumsum(e[:-1], out=off[1:])
    return off, int(e.sum())


def want_verdict(nodes, node_count, fallback, bad_index, long_nodes, level_end, node_cap):
    ok = fallback == 0 and bad_index == 0 and 0 < nodes <= node_cap and node_count <= node_cap and (level_end <= 0 or long_nodes == 0)
    return (nodes, 1) if ok else (0, 0)


def check_launch(C, hist, ids, shift, route, keep=False, build=ACCEPT, label=""):
    """One launch against the reference.  Returns (flagged, result)."""
    n = ids.size
    r = C.selftest_walk_estimate(hist, ids, shift=shift, route=route, keep_scratch=keep, clear_words=300, **build)
    off, total = reference(hist, ids, shift)
    flagged = total > LIMIT
    extra = extra_waves(n)
    assert (r["extra"], r["grid_waves"]) == (extra, extra + n // 64 + 4), label
    info = [int(x) for x in r["info"]]
    assert info[1] == int(flagged), (label, route, total, info)
    assert info[6] == 0 and info[7] == 0, label                       # the walk's own term count starts at zero
    assert info[4] == groups_of(route, n), (label, route, info)      # info[4] is each route's own: how many groups counted in
    if not flagged:
        budget = budget_of(total, extra, shift)
        # the grid rule of tile_total (a wave index the grid does not hold) cannot fire: total // budget <= extra
        assert total // budget + n // 64 + 1 < r["grid_waves"], label
        assert np.array_equal(r["off"].astype(U64), off), (label, route, int(np.flatnonzero(r["off"].astype(U64) != off)[0]))
        assert (info[0], info[3], info[5]) == (total, budget, total // budget + (n - 1) // 64), (label, route, total, info)
        # info[2] says "the 32-bit offsets wrapped" on routes 0 and 1 and repeats info[1] on route 2: alike only when unflagged
        assert info[2] == 0, (label, route, info)
    else:
        # offsets are not compared (32-bit sums wrap on routes 0 and 1 and saturate on route 2).  info[0] = min(total, 2^31 - 1)
        # holds on route 2 only: the saturating scan knows a clipped total, routes 0 and 1 take theirs from a wrapped 32-bit
        # offset (the value only reaches a trace line once info[1] is set) and guarantee no more than a clipped, non-negative int
        assert 0 <= info[0] <= LIMIT, (label, route, info)
        if route == 2:
            assert info[0] == LIMIT, (label, info)
    if route != 0:   # the tail's duties: verdict, the packed record verbatim, the build's counters cleared
        assert tuple(int(x) for x in r["verdict"]) == want_verdict(**build), (label, route, r["verdict"])
        assert np.array_equal(r["pack"], np.concatenate([r["verdict"], r["flags"], r["info"]])), (label, route)
        assert not r["clear"].any(), (label, route)
    return flagged, r


# ---- inputs: what each target's history holds (`vals`, by target), laid out in `hist` by `ids`
def _spread(total, n, shift, rng):
    """n values whose shifted sum is exactly `total`, the bits below the shift random; None if they cannot hold it."""
    top = 2 ** (32 - shift) - 1
    if total > n * top:
        return None
    q, rem = divmod(total, n)
    s = np.full(n, q, U64)
    s[:rem] += U64(1)
    assert int(s.max()) <= top and int(s.sum()) == total
    low = rng.integers(0, 2 ** shift, n).astype(U64)
    return ((s << U64(shift)) | low).astype(U32)


def contents(n, shift, rng):
    """(name, vals, whether the total is past 2^31 - 1 — known from how the values are made)."""
    out = [("zeros", np.zeros(n, U32), False), ("ones", np.ones(n, U32), False),
           ("random", rng.integers(0, 4001, n).astype(U32), False)]
    for where, t in (("first", 0), ("middle", n // 2), ("last", n - 1)):
        v = np.zeros(n, U32)
        v[t] = 2_000_000_000
        out.append((f"spike {where}", v, False))
    for name, total, flag in (("total 2^31 - 1", LIMIT, False), ("total 2^31", LIMIT + 1, True)):
        v = _spread(total, n, shift, rng)
        if v is not None:                                            # (n values of 32 - shift bits cannot always hold it)
            out.append((name, v, flag))
    out.append(("poison", np.full(n, 0xFFFFFFFF, U32), n * (0xFFFFFFFF >> shift) > LIMIT))   # (one target, shift 1: 2^31 - 1 exactly)
    if shift > 0:                                                    # the unshifted sum wraps 32 bits, the shifted sum fits
        total = min(LIMIT, n * (2 ** (32 - shift) - 1))
        s = _spread(total, n, shift, rng)
        v = (s.astype(U64) | U64(2 ** shift - 1)).astype(U32)
        assert n == 1 or int(v.astype(U64).sum()) >= 2 ** 32
        out.append(("wraps unshifted", v, False))
    return out


def layout(n, kind, rng):
    if kind == "permutation":                                        # every particle a target, in tree order
        return n, rng.permutation(n).astype(U32)
    return 2 * n, np.arange(1, 2 * n, 2, dtype=U32)                  # a shard's slice of a history twice as long


@pytest.mark.parametrize("kind", ["permutation", "strided"])
@pytest.mark.parametrize("n", SIZES)
def test_estimate_scans_equal_the_integer_reference(nb, n, kind):
    C = nb._capi
    rng = np.random.default_rng(1000 + n)
    big_n, ids = layout(n, kind, rng)
    for shift in (0, 1, 5):
        for name, vals, want_flag in contents(n, shift, rng):
            hist = np.full(big_n, 0xFFFFFFFF, U32)                   # what no target owns would wreck any sum that read it
            hist[ids] = vals
            _, total = reference(hist, ids, shift)
            # each case is flagged or not by construction; the reference's total must say the same before any kernel is asked
            assert (total > LIMIT) == want_flag, (name, n, shift, total)
            got = [check_launch(C, hist, ids, shift, route, label=f"{name} n={n} shift={shift} {kind}") for route in ROUTES]
            if not want_flag:                                        # the three routes agree where they mean the same
                for _, r in got[1:]:
                    assert [int(r["info"][k]) for k in (0, 1, 3, 5)] == [int(got[0][1]["info"][k]) for k in (0, 1, 3, 5)]
                    assert np.array_equal(r["off"], got[0][1]["off"])
            assert all(f == want_flag for f, _ in got)


def test_scan_state_is_reused_across_launches_by_epoch(nb):
    """The host zeroes the scan's state area once per allocation; every launch after that finds the tickets and states of
    the launches before it, of other group counts, and must not take one for its own (epochs).  One kept scratch, route-2
    launches of 1, 5, 67 and 1 025 work-groups in turn, the other two routes in between."""
    C = nb._capi
    rng = np.random.default_rng(77)
    sizes = {1: 700, 5: 4 * 1024 + 1, 67: 66 * 1024 + 1, 1025: 1024 * 1024 + 9}
    assert all(groups_of(2, n) == g for g, n in sizes.items())
    order = [1025] + [g for _ in range(10) for g in (1, 5, 67, 1025)][:-1] + [5, 1, 1, 67, 5]
    launches = 0
    for k, g in enumerate(order):
        n = sizes[g]
        ids = rng.permutation(n).astype(U32)
        hist = rng.integers(0, 1500, n).astype(U32)                  # (1.05 M x 1 500 stays below 2^31)
        flagged, r = check_launch(C, hist, ids, 0, 2, keep=True, label=f"launch {k}: {g} groups")
        assert not flagged and r["kept"] == (k > 0), k                # (the first call finds nothing kept and allocates)
        launches += 1
        if k % 3 == 1:
            for route in (1, 0):
                flagged, r = check_launch(C, hist[::-1].copy(), ids, 0, route, keep=True, label=f"launch {k}, route {route}")
                assert not flagged and r["kept"]
    assert launches >= 40
    flagged, r = check_launch(C, hist, ids, 0, 2, keep=False, label="last")   # a fresh block again; nothing stays allocated
    assert not flagged and not r["kept"]


@pytest.mark.parametrize("route", [1, 2])
def test_build_verdict_rejects_each_condition_alone(nb, route):
    """tile_tail_duties commits a speculated build only if nothing is wrong with it.  One accepting setting; each reject
    condition flipped alone; and the one condition that is skipped (no blind levels: level_end 0)."""
    C = nb._capi
    n = 3000
    ids = np.arange(n, dtype=U32)
    hist = (np.arange(n) % 50).astype(U32)
    base = dict(nodes=900, node_count=1000, fallback=0, bad_index=0, long_nodes=0, level_end=7, node_cap=1000)
    cases = [("accepts", {}, (900, 1)),
             ("as many nodes as fit", dict(nodes=1000), (1000, 1)),
             ("fallback", dict(fallback=1), (0, 0)),
             ("bad index", dict(bad_index=3), (0, 0)),
             ("no nodes", dict(nodes=0), (0, 0)),
             ("more nodes than fit", dict(nodes=1001), (0, 0)),
             ("more node ids than fit", dict(node_count=1001), (0, 0)),
             ("a long node left", dict(long_nodes=2), (0, 0)),
             ("no blind levels: not asked", dict(long_nodes=2, level_end=0), (900, 1))]
    for name, flip, want in cases:
        build = dict(base, **flip)
        assert want_verdict(**build) == want, name
        flagged, r = check_launch(C, hist, ids, 0, route, build=build, label=name)   # (verdict, pack and clear region checked there)
        assert not flagged and tuple(int(x) for x in r["verdict"]) == want, (name, r["verdict"])
        f = r["flags"]                                               # the block as built: the inputs where the build keeps them
        assert (f[0], f[1], f[7], f[16], f[32 + build["level_end"]]) == (build["fallback"], build["node_count"], build["bad_index"],
                                                                          build["nodes"], build["long_nodes"]), name
