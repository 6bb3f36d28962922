"""tests/_nearfar.py checked on the CPU: the restated rule against a brute-force count, the planted scene's figures, and the proof
that the scene covers every (cell parity, neighbour cell) case — a split that ignores any ONE of the 36 cannot give the scene's
near set.  No GPU."""
import numpy as np
import pytest

from tests import _nearfar as NF

F32 = np.float32


def _brute_near(pos):
    c = NF.cell(pos).astype(np.int64)
    cheb = np.abs(c[:, None, :] - c[None, :, :]).max(axis=2)
    np.fill_diagonal(cheb, 99)
    return (cheb <= 1).any(axis=1)


def test_cell_floors_towards_minus_infinity_and_reproduces_the_pitch():
    h, inv_h = NF.pitch()
    assert h == np.sqrt(np.float64(F32(0.001))) * 1.001 and inv_h == 1.0 / h and h > np.sqrt(0.001)
    pos = np.array([[0.0, -0.0], [1e-45, -1e-45], [0.5 * h, -0.5 * h], [1.5 * h, -1.5 * h]], F32)
    assert NF.cell(pos).tolist() == [[0, 0], [0, -1], [0, -1], [1, -2]]          # floor, not truncation


def test_in_range_is_strict_at_both_ends():
    b = float(NF.CELL_BIAS)
    c = np.array([[b - 3, 0], [b - 2, 0], [0, -b + 3], [0, -b + 2], [np.nan, 0], [0, np.inf]])
    assert NF.in_range(c).tolist() == [True, False, True, False, False, False]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restated_near_equals_a_brute_force_count(seed):
    rng = np.random.default_rng(seed)
    pos = ((rng.random((600, 2)) - 0.5) * 3.0).astype(F32)          # ~95 x 95 cells around the origin, both signs: about half are near
    got = NF.near(pos)
    assert np.array_equal(got, _brute_near(pos)) and 50 < got.sum() < 550
    mass = np.full(600, 3, F32)
    mass[[0, 599]] = 2, 4
    heavy = NF.near(pos, mass, heavy_base=3.0)
    assert np.array_equal(heavy, got | (mass != 3))


def test_expected_far_layout_and_flags():
    pos = np.arange(6, dtype=F32).reshape(3, 2) + 1          # bodies (1,2) (3,4) (5,6), body 1 near
    near = np.array([False, True, False])
    E = NF.FAR_POINT
    assert NF.expected_far(pos, near, couples=False).tolist() == [[1, 2], [E, E], [5, 6]]
    far = NF.expected_far(pos, near, couples=True)
    assert far.shape == (32,) and far[:8].tolist() == [1, E, 2, E, 5, E, 6, E] and np.all(far[8:] == E)
    assert NF.expected_minv(np.array([0, 1, 2.0 ** 32], F32)).tolist() == [np.inf, 1.0, 2.0 ** -32]
    assert NF.expected_flags(pos * 100, near, use_hazard=True) == (0, 0, 1, 1)          # 1 > 3 // 64
    assert NF.expected_flags(np.array([[1, 2.0 ** 60]], F32), [False], True) == (1, 1, 0, 2)
    assert NF.expected_flags(np.array([[1, 2.0 ** 60]], F32), [False], False) == (0, 1, 0, 1)


def test_outside_fast_at_its_edges():
    vals = np.array(NF.FAST_EDGE_VALUES, F32)
    assert len(vals) == 13
    #        2^60 -2^60  pred -pred  2^-22 -2^-22 pred  -pred  denorm -0.0   0.0    inf   nan
    want = [True, True, False, False, False, False, True, True, True, False, False, True, True]
    assert NF.outside_fast(vals).tolist() == want


def test_range_edge_values_straddle_the_edge():
    for sign in (1, -1):
        inside, outside = NF.range_edge(sign)
        assert np.nextafter(inside, F32(sign * np.inf)) == outside and abs(float(outside)) < 2.0 ** 60
        assert NF.in_range(NF.cell([[inside, 0]]))[0] and not NF.in_range(NF.cell([[outside, 0]]))[0]
        assert abs(NF.cell([[inside, 0]])[0, 0]) > NF.CELL_BIAS - 100          # within one f32 step of the edge


def test_planted_scene_figures():
    """848 planted bodies, 336 of them near and nothing else; all 36 cases present; the nearest far pair is farther apart than
    sqrt(clamp) and the near pairs well inside it; state 0 is reachable at N_SCENE."""
    cells, fracs, pairs = NF.planted_pairs()
    assert len(cells) == 848 and len(pairs) == 424
    pos, rows = NF.planted_scene()
    n = len(pos)
    assert n == NF.N_SCENE == 24576
    near = NF.near(pos)
    want = np.zeros(n, bool)
    cases = set()
    dist_near, dist_far = [], []
    for a, b, par, d in rows:
        cheb = max(abs(d[0]), abs(d[1]))
        dist = float(np.hypot(*(pos[a].astype(np.float64) - pos[b])))
        if cheb <= 1:
            want[[a, b]] = True
            cases.add(par + d)
            dist_near.append(dist)
        else:
            dist_far.append(dist)
    assert np.array_equal(near, want) and near.sum() == 336 <= n // 64 and near.sum() > 20480 // 64
    assert cases == set(NF.CASES) and len(cases) == 36
    r = np.sqrt(0.001)
    print(f"near pairs {min(dist_near):.4f} .. {max(dist_near):.4f}, nearest far pair {min(dist_far):.4f}, sqrt(clamp) {r:.4f}, "
          f"largest |cell| {np.abs(NF.cell(pos)).max():.0f}")
    assert 0.006 < min(dist_near) and max(dist_near) < 0.5 * r and min(dist_far) > 1.15 * r
    assert NF.expected_flags(pos, near, True) == (0, 0, 336, 0)
    c = NF.cell(pos)
    assert (c[:, 0] < 0).sum() > 400 and (c[:, 1] < 0).sum() > 400 and {-1.0, 0.0} <= set(c[:, 0]) and {-1.0, 0.0} <= set(c[:, 1])


@pytest.mark.parametrize("case", NF.CASES, ids=lambda c: "p%d%d_d%+d%+d" % c)
def test_every_case_decides_the_scenes_near_set(case):
    """The rule with one neighbour cell deleted for one cell parity gives ANOTHER near set on this scene: a classifier that
    misses that case cannot pass the set comparison."""
    pos, _ = _scene()
    full = _scene_near()
    miss = NF.near(pos, skip=case)
    assert np.all(full[miss]) and (full & ~miss).sum() >= 4          # (one body per base at the least)


_CACHE = {}


def _scene():
    if "scene" not in _CACHE:
        _CACHE["scene"] = NF.planted_scene()
    return _CACHE["scene"]


def _scene_near():
    if "near" not in _CACHE:
        _CACHE["near"] = NF.near(_scene()[0])
    return _CACHE["near"]


@pytest.mark.parametrize("n_near", [0, 63, 64, 65, 129, 255, 256, 257, 383, 384, 385])
def test_counted_scenes_hold_exactly_that_many_near_bodies(n_near):
    pos = NF.counted_scene(n_near)
    assert len(pos) == NF.N_SCENE and NF.near(pos).sum() == n_near
    assert NF.expected_flags(pos, NF.near(pos), True)[3] == (1 if n_near > 384 else 0)


def test_the_door_is_declared_and_bound(nb):
    C = nb._capi
    assert "nbody_selftest_nearfar" in C.declared_symbols() and "nbody_selftest_nearfar" in C._SIGS
    assert len(C._SIGS["nbody_selftest_nearfar"][1]) == 15
