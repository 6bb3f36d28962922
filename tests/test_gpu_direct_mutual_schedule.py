"""The mutual main pass's schedule (csrc/mutual_schedule.h): units of equal cost — an off-diagonal slice pair, or two diagonal
slices each taken mutually — in strips of whole rounds.  Sizes that leave every kind of remainder: the crossover, 2^20 (8192
units, 32 rounds), an odd slice count, a partial last slice, 3 x 2^20 and the 2^22 bound.  Each scene puts coincident and
clamp-radius bodies inside one slice, in the wave-block pairs the diagonal shares out differently (own block, distance 1 .. 3, and
the split distance 4), and in one couple.  Within the FAST contract against the oracle, bitwise reproducible.  Needs an MI355X."""
import numpy as np
import pytest

from tests._tol import check_fast

pytestmark = pytest.mark.gpu
F32 = np.float32
SLICE = 8192          # bodies per slice; a wave block is 1024 of them


@pytest.fixture(scope="module")
def ctx(nb):
    c = nb._capi.Context(0)
    yield c
    c.close()


def _scene(nb, n, seed):
    pos, vel, w = nb.scenes.plummer(n, seed=seed)
    s0 = SLICE * (n // SLICE // 2)                         # a slice in the middle of the problem
    special = []
    for a, b, off in [(10, 11, 0.0),                       # one couple, coincident
                      (100, 900, 0.0),                     # one wave block, coincident
                      (1030, 3100, 0.0078125),             # wave blocks 1 and 3, clamp radius
                      (500, 4600, 0.0),                    # blocks 0 and 4 (the split pair), coincident
                      (5200, 1300, 0.0078125),             # blocks 5 and 1 (the split pair, other way)
                      (7000, 200, 0.5)]:                   # blocks 6 and 0 (distance 2 from the upper side), close
        pos[s0 + a] = pos[s0 + b] + F32(off)
        special += [s0 + a, s0 + b]
    return pos, vel, w, special


def _accel(ctx, C, pos, vel, w):
    ctx.set_params(arith=C.ARITH_AUTO, clamp=0.001)
    ctx.upload(pos, vel, w)
    return ctx.accel_direct()


@pytest.mark.parametrize("n", [393216, 1 << 20, (1 << 20) + 12345, 3 << 20, 1 << 22])
def test_mutual_schedule_sizes(nb, orc, ctx, n):
    C = nb._capi
    pos, vel, w, special = _scene(nb, n, seed=90 + n % 7)
    a = _accel(ctx, C, pos, vel, w)
    stride = max(n // 600, 1) | 1
    tg = np.unique(np.concatenate([np.arange(0, n, stride), special, [0, n - 1]]))
    ref64, norm = orc.direct_accel(pos, w, targets=tg, accum="f64", nthreads=16)
    check_fast(a[tg], ref64, norm, label=f" mutual n={n}")
    assert np.array_equal(a, _accel(ctx, C, pos, vel, w))
