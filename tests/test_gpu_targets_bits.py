"""A tracer's value is the probe call's, bit for bit — FAST included.

The probe call (Context.accel_direct(targets)) and the tracers' share of a direct step run the same kernels (target_kernels.hip)
with different output policies; the other tests check FAST against a tolerance only, so nothing else would notice the two
drifting apart by a rounding.  One case: the acceleration `a` at the targets from the probe call; then the same points as tracers
at rest, one direct step with dt = 1.  The step computes v1 = 0 + a * 1 and x1 = x0 + v1 * 1, so the downloaded rows must equal
those two expressions evaluated in numpy from the probe call's `a`, byte for byte (0 + a turns a -0 term into the step's +0).

Bodies: 1, 255 and 257 (one LDS stage of 256 short by one, and one over), 8193 (two f32 FAST splits, three f64).  Targets: one
exactly on a body (the skipped pair), one outside FAST's domain (where f32 AUTO and f64 FAST route per target, the device's marks
and the host's scan must pick the same points), the rest near the bodies.  Needs an MI355X."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
OUTSIDE = {F32: 1e-30, F64: 1e-305}  # below 2^-22 and 2^-300: outside FAST's domain, a normal number


@pytest.fixture(scope="module")
def ctx(nb):
    c = nb._capi.Context(0)
    yield c
    c.close()


def _bytes_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("m", [1, 257])
@pytest.mark.parametrize("n", [1, 255, 257, 8193])
@pytest.mark.parametrize("dt,arith", [(F32, "fast"), (F32, "auto"), (F32, "exact"), (F64, "fast"), (F64, "exact")])
def test_a_tracer_step_from_rest_is_the_probe_calls_acceleration(nb, ctx, dt, arith, n, m):
    C = nb._capi
    rng = np.random.default_rng(1000 * n + m)
    pos, vel, w = nb.scenes.plummer(n, seed=0x7A6 + n, dtype=dt)
    if n >= 255:
        w = rng.integers(1, 1000, n).astype(np.uint32)
    tgt = (pos[rng.integers(0, n, m)] + rng.normal(0, 0.5, (m, 2))).astype(dt)
    tgt[0] = pos[n // 2]  # exactly on a body
    if m > 1:
        tgt[m // 2, 0] = OUTSIDE[dt]
    ctx.set_params(arith={"auto": C.ARITH_AUTO, "fast": C.ARITH_FAST, "exact": C.ARITH_EXACT}[arith])  # (the default clamp, 0.001)
    ctx.upload(pos, vel, w)
    a = ctx.accel_direct(tgt)
    assert a.dtype == dt and np.all(np.isfinite(a))
    ctx.upload_tracers(tgt, np.zeros_like(tgt))
    ctx.update_direct(1.0, 1)
    x1, v1 = ctx.download_tracers()
    one = dt(1)
    want_v = np.zeros_like(a) + a * one
    want_x = tgt + want_v * one
    assert want_v.dtype == dt and want_x.dtype == dt
    assert _bytes_equal(v1, want_v), np.flatnonzero((v1 != want_v).any(axis=1))[:8]
    assert _bytes_equal(x1, want_x), np.flatnonzero((x1 != want_x).any(axis=1))[:8]
