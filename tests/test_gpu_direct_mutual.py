"""The mutual main pass of the direct step (csrc/direct_mutual.hip: each far pair evaluated once, Newton's third law) against the
oracle and against the one-sided streamed pass.  It engages for FAST arithmetic with equal masses (or one mass but for a few
bodies), one block of targets covering every source, and 393 216 <= n <= 4 194 304 (the lower bound: lab NBODY_DIRECT_MUTUAL_MIN_N).
Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests._tol import check_fast

pytestmark = pytest.mark.gpu
F32 = np.float32
N_ODD = 393216 + 4099          # just above the crossover; not a multiple of 128, of 16 or of a slice (8192)


@pytest.fixture(scope="module")
def ctx(nb):
    c = nb._capi.Context(0)
    yield c
    c.close()


def _scene(nb, n, seed):
    pos, vel, w = nb.scenes.plummer(n, seed=seed)
    pos[100] = pos[200]                                    # coincident: contributes nothing
    pos[300] = pos[400] + F32(0.0078125)                   # inside the clamp radius: near bodies
    return pos, vel, w


def _accel(ctx, C, pos, vel, w):
    ctx.set_params(arith=C.ARITH_AUTO, clamp=0.001)
    ctx.upload(pos, vel, w)
    return ctx.accel_direct()


@pytest.mark.parametrize("heavy", [False, True])
def test_mutual_within_contract_and_differs_from_streamed(nb, orc, lab_ctx, monkeypatch, heavy):
    """Lab NBODY_DIRECT_ASM=4 (mutual) and =3 (direct_stream) both within the frozen tolerance of the oracle's f64 sum, on every
    sampled target including the coincident and near ones; their bits differ (the mutual pass ran); two calls agree bit for bit.
    heavy: two heavy bodies as in the reference scene (the equal-mass rate with the odd masses in the near list)."""
    C = nb._capi
    pos, vel, w = _scene(nb, N_ODD, 81)
    if heavy:
        w = w.copy()
        w[0], w[1] = 75_000_000, 750_000
    tg = np.unique(np.concatenate([np.arange(0, N_ODD, 997), [0, 1, 100, 200, 300, 400, N_ODD - 1]]))
    ref64, norm = orc.direct_accel(pos, w, targets=tg, accum="f64", nthreads=16)
    got = {}
    for mode in ("3", "4"):
        monkeypatch.setenv("NBODY_DIRECT_ASM", mode)
        got[mode] = _accel(lab_ctx, C, pos, vel, w)
        check_fast(got[mode][tg], ref64, norm, label=f" NBODY_DIRECT_ASM={mode}")
    assert not np.array_equal(got["3"], got["4"])
    monkeypatch.setenv("NBODY_DIRECT_ASM", "4")
    assert np.array_equal(got["4"], _accel(lab_ctx, C, pos, vel, w))


def test_reference_scene_through_the_mutual_pass(nb, orc, lab_ctx, monkeypatch):
    """The reference's own scene (galaxy(): ~151 000 bodies, two heavy ones that travel with the near list), below the crossover,
    with the lab's lower bound lifted: the mutual pass (ASM 4) and direct_stream (ASM 3) both within the contract, different bits."""
    C = nb._capi
    pos, vel, w = nb.scenes.galaxy()
    n = len(pos)
    tg = np.unique(np.concatenate([np.arange(0, n, 331), [0, 1, n - 1]]))
    ref64, norm = orc.direct_accel(pos, w, targets=tg, accum="f64", nthreads=16)
    monkeypatch.setenv("NBODY_DIRECT_MUTUAL_MIN_N", "0")
    got = {}
    for mode in ("3", "4"):
        monkeypatch.setenv("NBODY_DIRECT_ASM", mode)
        got[mode] = _accel(lab_ctx, C, pos, vel, w)
        check_fast(got[mode][tg], ref64, norm, label=f" galaxy NBODY_DIRECT_ASM={mode}")
    assert not np.array_equal(got["3"], got["4"])


def _streamed(nb, C, pos, vel, w, monkeypatch):
    """The same call through direct_stream (lab ASM 3): what the product would give without the mutual pass."""
    monkeypatch.setenv("NBODY_DIRECT_ASM", "3")
    with nb._capi.laboratory():
        with nb._capi.Context(0) as c:
            return _accel(c, nb._capi, pos, vel, w)


@pytest.mark.parametrize("n", [1 << 20, (1 << 21) + 12345])
def test_mutual_at_large_sizes(nb, orc, ctx, monkeypatch, n):
    """The headline's size and an odd size past it (over a hundred strips of items), sampled targets; the product library's
    answer is not direct_stream's (the mutual pass engaged there) and is reproducible."""
    C = nb._capi
    pos, vel, w = nb.scenes.plummer(n, seed=82)
    a = _accel(ctx, C, pos, vel, w)
    tg = np.arange(0, n, 4099)
    ref64, norm = orc.direct_accel(pos, w, targets=tg, accum="f64", nthreads=16)
    check_fast(a[tg], ref64, norm, label=f" mutual n={n}")
    assert np.array_equal(a, _accel(ctx, C, pos, vel, w))
    assert not np.array_equal(a, _streamed(nb, C, pos, vel, w, monkeypatch))


def test_hazardous_position_still_takes_exact(nb, orc, ctx):
    """A coordinate outside FAST's domain sends the step to EXACT on the device, bit-identical to the oracle."""
    C = nb._capi
    pos, vel, w = nb.scenes.plummer(N_ODD, seed=83)
    pos[777, 1] = 2.0 ** 61
    a = _accel(ctx, C, pos, vel, w)
    tg = np.arange(0, N_ODD, 8191)
    ref, _ = orc.direct_accel(pos, w, targets=tg, nthreads=16)
    assert np.array_equal(a[tg], ref.astype(F32))


def test_single_rank_stepper_equals_context_path_mutual(nb, monkeypatch):
    """The device-pointer route (ShardedDirectStepper, world = 1: the benchmark's) chooses the mutual pass like the context route."""
    from nbody_simulation_amd.sharding import ShardedDirectStepper
    C = nb._capi
    pos, vel, w = _scene(nb, N_ODD, 84)
    st = ShardedDirectStepper(pos, vel, w, device=torch.device("cuda", 0), arith=C.ARITH_AUTO)
    st.step(0.1)
    torch.cuda.synchronize()
    p, v = st.local_state()
    with C.Context(0) as c:
        c.upload(pos, vel, w)
        c.update_direct(0.1, 1)
        cp, cv, _, _ = c.download()
    assert np.array_equal(p, cp) and np.array_equal(v, cv)
    monkeypatch.setenv("NBODY_DIRECT_ASM", "3")            # ... and that path is the mutual pass, not direct_stream
    with C.laboratory():
        with C.Context(0) as c:
            c.upload(pos, vel, w)
            c.update_direct(0.1, 1)
            sp, sv, _, _ = c.download()
    assert not (np.array_equal(p, sp) and np.array_equal(v, sv))
