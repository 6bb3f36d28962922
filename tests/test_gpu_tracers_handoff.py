"""Tracers in the hand-off: the frame with tracers (nbody_render_rgba_tracers), the snapshot's tracers (nbody_snapshot_tracers_*)
and the tracers' delta stream (nbody_tracers_delta_*).

Every comparison is exact, in bytes and bits: frames against the oracle's draw() over the bodies' rows followed by the tracers as
rows of weight 1, streams against the numpy statement of the format (oracle/delta_codec.py) fed the tracers' positions, snapshots
against the library's own synchronous download.  Needs an MI355X."""
import numpy as np
import pytest

from oracle import delta_codec as dc

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
HEIGHT = 100_000


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _draw_with_tracers(orc, p, v, w, tp, tv, height=HEIGHT, px=1250):
    return orc.draw(np.concatenate([p, tp]), np.concatenate([v, tv]), np.concatenate([w, np.ones(len(tp), np.uint32)]), height, px)


def _bodies_and_tracers(nb, n, m, dtype, seed=77):
    """n bodies and m tracers: consecutive members of one seeded Plummer set."""
    pos, vel, w = nb.scenes.plummer(n + m, seed=seed, dtype=dtype)
    return pos[:n], vel[:n], w[:n], np.ascontiguousarray(pos[n:]), np.ascontiguousarray(vel[n:])


# ------------------------------------------------------------------------------------------------ frame
def _crowded_scene():
    """3 000 bodies and 5 000 tracers (f64 values that are exact in f32).  60 hot pixels of the 1250-frame inside the patch
    [40 000, 42 000)^2 take 15 bodies and 20 tracers each — under 25 rows of either kind, over 25 together — on top of a uniform
    fill of the patch; the rest lies all over and beyond the frame."""
    rng = np.random.default_rng(2024)
    n, m, cell = 3000, 5000, 80
    idx = rng.choice(25 * 25, 60, replace=False)
    hot = np.stack([40_000 + cell * (idx % 25), 40_000 + cell * (idx // 25)], axis=1).astype(F64)

    def place(k_hot, k_patch, k_all):
        a = np.repeat(hot, k_hot, axis=0) + rng.random((60 * k_hot, 2)) * cell
        b = rng.random((k_patch, 2)) * 2000 + 40_000
        c = rng.random((k_all, 2)) * 1.1e5 - 5e3
        return np.concatenate([a, b, c]).astype(F32).astype(F64)

    pos = place(15, 1100, 1000)
    tpos = place(20, 1800, 2000)
    assert pos.shape == (n, 2) and tpos.shape == (m, 2)
    vel = (rng.standard_normal((n, 2)) * 4).astype(F32).astype(F64)
    tvel = (rng.standard_normal((m, 2)) * 4).astype(F32).astype(F64)
    w = np.where(rng.random(n) < 0.03, 11, 10).astype(np.uint32)       # 10 / 11 straddle "> 10"
    pos[-5:] = tpos[[0, 20, 1300, 3100, 3101]]                         # heavy bodies on pixels that tracers hit: hot, patch, anywhere
    w[-5:] = 750_000
    tpos[3200] = (-40.0, 500.0)                                        # outside [0, HEIGHT)^2 (others of the spread are too)
    tpos[3201] = (500.0, 100_000.0)
    tpos[3202] = (np.nan, 10.0)
    tpos[-2:] = tpos[[45, 65]]                                         # the last rows of two hot pixels: their colour is the pixel's
    tvel[-2] = (np.inf, 0.0)
    tvel[-1] = (np.nan, 0.0)
    return pos, vel, w, tpos, tvel


def _light_counts(p, light, px):
    cell = HEIGHT // px
    ok = light & np.all((p >= 0) & (p < HEIGHT), axis=1)
    q = p[ok].astype(np.int64) // cell
    return np.bincount(q[:, 1] * px + q[:, 0], minlength=px * px)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_frame_with_tracers_equals_draw_of_bodies_then_tracers_on_crowded_pixels(nb, orc, dtype):
    C = nb._capi
    pos, vel, w, tpos, tvel = (a if a.dtype == np.uint32 else a.astype(dtype) for a in _crowded_scene())
    # the inputs do what they are for: pixels whose alpha saturates only with bodies and tracers counted together
    cb, ct = _light_counts(pos, w <= 10, 1250), _light_counts(tpos, np.ones(len(tpos), bool), 1250)
    heavy = _light_counts(pos, w > 10, 1250) > 0
    assert np.count_nonzero((cb < 25) & (cb > 0) & (ct < 25) & (ct > 0) & (cb + ct > 25) & ~heavy) >= 10
    assert np.count_nonzero(heavy & (ct > 0)) >= 3
    with C.Context(0) as ctx:
        ctx.upload(pos, vel, w)
        ctx.upload_tracers(tpos, tvel)
        for px in (1250, 100):
            want = _draw_with_tracers(orc, pos, vel, w, tpos, tvel, HEIGHT, px)
            bodies_only = orc.draw(pos, vel, w, HEIGHT, px)
            assert not np.array_equal(want, bodies_only), px            # a no-op implementation cannot pass
            assert np.array_equal(ctx.render(HEIGHT, px, tracers=True), want), px
            assert np.array_equal(ctx.render(HEIGHT, px), bodies_only), px   # the existing call: bodies only, as ever


def test_frame_with_tracers_follows_the_bodies_row_order_and_the_tracers_upload_order(nb, orc):
    """The bodies are permuted by every BVH build, the tracers never: rows = particles() followed by tracers()."""
    pos, vel, w = nb.scenes.galaxy()
    assert list(w[:2]) == [75_000_000, 750_000]
    nbod = 2 + 2000
    world = nb.World(pos[:nbod], vel[:nbod], w[:nbod], method="bvh", tracers=(pos[nbod:nbod + 20_000], vel[nbod:nbod + 20_000]))
    try:
        cnt = nb.Counting()
        for _ in range(3):
            world.update(0.1, cnt)
        p, v, w2, ids = world.particles()
        assert not np.array_equal(ids, np.arange(nbod))
        tp, tv = world.tracers()
        frame = world.frame(tracers=True)
        assert np.array_equal(frame, _draw_with_tracers(orc, p, v, w2, tp, tv))
        assert not np.array_equal(frame, world.frame())
        assert (frame[..., 1] == 255).any()                                # the heavy bodies stay green
    finally:
        world.close()


def test_frame_with_tracers_edges(nb):
    C = nb._capi
    with C.Context(0) as ctx:
        pos, vel = np.array([[85, 170]], F32), np.array([[0.3, -0.4]], F32)
        ctx.upload(pos, vel, np.ones(1, np.uint32))
        assert np.array_equal(ctx.render(tracers=True), ctx.render())      # m == 0
        assert tuple(ctx.render(tracers=True)[2, 1]) == (255, 232, 232, 10)
        ctx.upload_tracers(np.array([[90, 200]], F32), np.array([[1.0, 0.5]], F32))   # same pixel, v = 0x10 + 15
        f = ctx.render(tracers=True)
        assert tuple(f[2, 1]) == (255, 224, 224, 20) and np.count_nonzero(f) == 4
        assert tuple(ctx.render()[2, 1]) == (255, 232, 232, 10)
        with pytest.raises(C.NBodyError) as e:
            ctx.render(HEIGHT, 1251, tracers=True)                         # does not divide HEIGHT, as for nbody_render_rgba
        assert e.value.code == C.ERR_INVALID
        ctx.upload_tracers(np.zeros((1 << 24, 2), F32), np.zeros((1 << 24, 2), F32))   # rows 0 .. 2^24: one too many for the packing
        with pytest.raises(C.NBodyError, match="tracers") as e:
            ctx.render(tracers=True)
        assert e.value.code == C.ERR_INVALID
        assert tuple(ctx.render()[2, 1]) == (255, 232, 232, 10)            # the bodies' frame is not concerned


# ------------------------------------------------------------------------------------------------ snapshot
@pytest.mark.parametrize("method,dtype", [("direct", F32), ("quad", F64)])
def test_snapshot_tracers_are_the_state_at_begin(nb, method, dtype):
    pos, vel, w, tp, tv = _bodies_and_tracers(nb, 1000, 777, dtype)
    world = nb.World(pos, vel, w, method=method, tracers=(tp, tv))
    plain = nb.World(pos, vel, w, method=method, tracers=(tp, tv))      # the same run without the new call
    try:
        cnt = nb.Counting()
        for wd in (world, plain):
            wd.update(0.1, cnt)
        at_begin = world.tracers()
        assert not _same_bits(at_begin[0], tp)
        for wd in (world, plain):
            wd.snapshot_begin()
            wd.update(0.1, cnt, n_steps=2)
        assert world.ctx.lib.nbody_snapshot_num_tracers(world.ctx.h) == 777
        got = world.snapshot_tracers()
        assert _same_bits(got[0], at_begin[0]) and _same_bits(got[1], at_begin[1])
        assert not _same_bits(world.tracers()[0], at_begin[0])             # the steps went on meanwhile
        again = world.snapshot_tracers()                                   # it does not end the snapshot
        assert _same_bits(again[0], at_begin[0]) and world.ctx.snapshot_pending()
        a, b = world.snapshot_end(), plain.snapshot_end()
        assert a[4] == b[4] == 1
        for x, y in zip(a[:4], b[:4]):
            assert _same_bits(x, y)
        assert not world.ctx.snapshot_pending()
    finally:
        world.close()
        plain.close()


def test_snapshot_tracers_lifecycle(nb):
    C = nb._capi
    pos, vel, w, tp, tv = _bodies_and_tracers(nb, 300, 200, F32)
    with C.Context(0) as ctx:
        num = lambda: ctx.lib.nbody_snapshot_num_tracers(ctx.h)  # noqa: E731
        ctx.upload(pos, vel, w)
        ctx.upload_tracers(tp, tv)
        assert num() == 0
        with pytest.raises(C.NBodyError) as e:
            ctx.snapshot_tracers()                                         # nothing pending
        assert e.value.code == C.ERR_INVALID
        buf = np.zeros((200, 2), F32)
        assert ctx.lib.nbody_snapshot_tracers_f32(ctx.h, C._ptr(buf), None) == C.ERR_INVALID
        ctx.update_direct(0.1, 1)
        want = ctx.download_tracers()
        ctx.snapshot_begin()
        assert ctx.lib.nbody_snapshot_tracers_f64(ctx.h, None, None) == C.ERR_INVALID   # the other precision
        ctx.upload_tracers(np.zeros((0, 2), F32), np.zeros((0, 2), F32))   # the tracers go; the pending copy stays
        assert ctx.n_tracers == 0 and num() == 200
        ctx.update_direct(0.1, 1)
        got = ctx.snapshot_tracers()
        assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
        only_vel = np.zeros((200, 2), F32)
        assert ctx.lib.nbody_snapshot_tracers_f32(ctx.h, None, C._ptr(only_vel)) == C.OK    # either pointer may be NULL
        assert _same_bits(only_vel, want[1])
        ctx.snapshot_end()
        assert num() == 0
        ctx.snapshot_begin()                                               # a snapshot of a context without tracers
        assert num() == 0
        p, v = ctx.snapshot_tracers()
        assert p.shape == v.shape == (0, 2)
        assert ctx.lib.nbody_snapshot_tracers_f32(ctx.h, None, None) == C.OK
        ctx.snapshot_end()
        ctx.upload_tracers(tp[:50], tv[:50])                               # a body upload (which removes the tracers) neither
        ctx.snapshot_begin()
        ctx.upload(pos[:10], vel[:10], w[:10])
        assert ctx.n_tracers == 0 and num() == 50
        got = ctx.snapshot_tracers()
        assert _same_bits(got[0], tp[:50]) and _same_bits(got[1], tv[:50])
        assert ctx.lib.nbody_snapshot_end_f32(ctx.h, None, None, None, None, None) == C.OK   # (300 rows: Context.snapshot_end sizes for 10)


# ------------------------------------------------------------------------------------------------ delta
@pytest.mark.parametrize("m", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("method,dtype", [("direct", F32), ("bvh", F64)])
def test_tracer_stream_equals_the_format_statement(nb, method, dtype, m):
    pos, vel, w, tp, tv = _bodies_and_tracers(nb, 500, m, dtype)
    world = nb.World(pos, vel, w, method=method, tracers=(tp, tv))
    enc, dec = dc.Encoder(), nb.DeltaDecoder()
    try:
        cnt = nb.Counting()
        for k in range(5):
            if k:
                world.update(0.1, cnt)
            world.tracers_delta_begin()
            assert world.ctx.tracers_delta_pending() and not world.ctx.delta_pending()
            stream, step = world.tracers_delta_end()
            assert not world.ctx.tracers_delta_pending()
            now = world.tracers()[0]
            assert step == k and stream[5] == (1 if k == 0 else 0)
            assert stream == enc.encode(now, step=k)
            dec.apply(stream)
            assert dec.n == m and _same_bits(dec.positions(), now)
    finally:
        world.close()


def test_bodies_streams_do_not_notice_the_tracers_or_their_stream(nb):
    pos, vel, w, tp, tv = _bodies_and_tracers(nb, 2000, 1500, F32)
    with_tr = nb.World(pos, vel, w, method="bvh", tracers=(tp, tv))
    busy = nb.World(pos, vel, w, method="bvh", tracers=(tp, tv))          # a tracer stream pending around every bodies' stream
    without = nb.World(pos, vel, w, method="bvh")
    enc, dec = dc.Encoder(), nb.DeltaDecoder()
    try:
        cnt = nb.Counting()
        for k in range(4):
            if k:
                for wd in (with_tr, busy, without):
                    wd.update(0.1, cnt)
            for wd in (with_tr, without):
                wd.delta_begin()
            a, b = with_tr.delta_end(), without.delta_end()
            assert a == b
            first = ("tracers", "bodies") if k % 2 else ("bodies", "tracers")   # begin and end in either order
            for which in first:
                busy.tracers_delta_begin() if which == "tracers" else busy.delta_begin()
            assert busy.ctx.delta_pending() and busy.ctx.tracers_delta_pending()
            got = {}
            for which in (first if k < 2 else first[::-1]):
                got[which] = busy.tracers_delta_end() if which == "tracers" else busy.delta_end()
            assert got["bodies"] == a
            assert got["tracers"] == (enc.encode(busy.tracers()[0], step=k), k)
            dec.apply(got["tracers"][0])
            assert _same_bits(dec.positions(), busy.tracers()[0])
    finally:
        for wd in (with_tr, busy, without):
            wd.close()


def test_tracer_stream_lifecycle(nb):
    C = nb._capi
    pos, vel, w, tp, tv = _bodies_and_tracers(nb, 400, 1000, F32)
    with C.Context(0) as ctx:
        ctx.upload(pos, vel, w)
        with pytest.raises(C.NBodyError) as e:
            ctx.tracers_delta_begin()                                      # no tracers
        assert e.value.code == C.ERR_INVALID
        with pytest.raises(C.NBodyError):
            ctx.tracers_delta_end()                                        # nothing pending
        ctx.upload_tracers(tp, tv)
        ctx.tracers_delta_begin()
        with pytest.raises(C.NBodyError) as e:
            ctx.tracers_delta_begin()                                      # one in flight
        assert e.value.code == C.ERR_INVALID
        with pytest.raises(C.NBodyError, match="smaller than the stream"):
            ctx.tracers_delta_end(cap=64)
        assert ctx.tracers_delta_pending()                                 # still there
        with pytest.raises(C.NBodyError):
            ctx.tracers_delta_reset()
        s0, _ = ctx.tracers_delta_end()
        assert len(s0) <= ctx.lib.nbody_delta_bound(1000, 0)
        ctx.update_direct(0.1, 1)
        ctx.tracers_delta_begin()
        s1, _ = ctx.tracers_delta_end()
        ctx.tracers_delta_reset()
        ctx.tracers_delta_begin()
        s2, step2 = ctx.tracers_delta_end()
        assert (s0[5], s1[5], s2[5]) == (1, 0, 1) and step2 == 1
        d = nb.DeltaDecoder()
        d.apply(s2)                                                        # a key frame stands alone
        assert _same_bits(d.positions(), ctx.download_tracers()[0])
        assert s2 == dc.Encoder().encode(ctx.download_tracers()[0], step=1)
        for m in (100, 1000, 0, 1000):                                     # another m, the same m, none: a new sequence every time
            ctx.upload_tracers(tp[:m], tv[:m])
            if m == 0:
                with pytest.raises(C.NBodyError):
                    ctx.tracers_delta_begin()
                continue
            ctx.tracers_delta_begin()
            s3, _ = ctx.tracers_delta_end()
            assert s3[5] == 1 and s3 == dc.Encoder().encode(tp[:m], step=1)
            d = nb.DeltaDecoder()
            d.apply(s3)
            assert d.n == m and _same_bits(d.positions(), tp[:m])
        ctx.delta_begin()                                                  # the bodies' sequence starts with its own key frame
        assert ctx.delta_end()[0][5] == 1
