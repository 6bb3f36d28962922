"""Delta streams of an ensemble (nbody_deltas_*, ensemble_deltas.hip) on the device: every world's stream against the numpy
statement of the format (oracle/delta_codec.py) fed that world's downloaded rows alone, byte for byte, on all eight handles; the
independence of a world's bytes from its neighbours; the state left alone; the commit rule and the refusals.  Needs an MI355X.

The sizes are where this encoder can go wrong: partial last blocks (63, 65, 130), one-row worlds, worlds of exactly one block,
a segment of several blocks (4096, 5000), empty segments (a world without tracers), and in f64 widths up to 64."""
import ctypes

import numpy as np
import pytest

from oracle import delta_codec as dc

pytestmark = pytest.mark.gpu

GAPS = (0, 1, 1, 3, 1)                       # the uneven cadence of tests/test_gpu_delta.py
RAGGED_SIZES = [1, 64, 65, 130, 63, 4096]
RAGGED_TRACERS = [0, 1, 5000, 64, 0, 65]
WORDS = {"ensemble": "ensemble", "ensemble64": "ensemble", "ragged": "ragged", "ragged64": "ragged", "restricted": "restricted",
         "restricted64": "restricted", "rr": "ragged restricted", "rr64": "ragged restricted"}


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _rows(n, dtype, rng, special=False):
    pos = (rng.random((n, 2)) * 1000.0).astype(dtype)
    vel = rng.standard_normal((n, 2)).astype(dtype)
    if special:   # NaN, +-inf and -0.0 among the positions (as many as there is room for)
        flat = pos.reshape(-1)
        for i, v in enumerate([np.nan, np.inf, -np.inf, -0.0][:flat.size]):
            flat[(i * 5) % flat.size] = v
    return pos, vel


def _make(nb, handle, sizes, tracers, dtype, seed, arith="auto", special_world=1):
    """The class of `handle` over worlds of `sizes` bodies (uniform handles: all equal) and `tracers` tracers (None: none),
    world `special_world` holding the special values."""
    rng = np.random.default_rng(seed)
    worlds = [_rows(n, dtype, rng, special=k == special_world) for k, n in enumerate(sizes)]
    tr = None if tracers is None else [_rows(m, dtype, rng, special=k == special_world) for k, m in enumerate(tracers)]
    pos, vel = [w[0] for w in worlds], [w[1] for w in worlds]
    base = handle.rstrip("64")
    f64 = handle.endswith("64")
    if base == "ensemble":
        return (nb.Ensemble64 if f64 else nb.Ensemble)(np.stack(pos), np.stack(vel), arith=arith)
    if base == "restricted":
        t = None if tr is None else (np.stack([t[0] for t in tr]), np.stack([t[1] for t in tr]))
        return (nb.RestrictedEnsemble64 if f64 else nb.RestrictedEnsemble)(np.stack(pos), np.stack(vel), tracers=t, arith=arith)
    if base == "ragged":
        return (nb.RaggedEnsemble64 if f64 else nb.RaggedEnsemble)(pos, vel, arith=arith)
    return (nb.RaggedRestrictedEnsemble64 if f64 else nb.RaggedRestrictedEnsemble)(pos, vel, tracers=tr, arith=arith)


def _body_rows(ens):
    p = ens.particles()[0]
    return [np.ascontiguousarray(w) for w in p]


def _tracer_rows(ens):
    t = ens.tracers()
    if isinstance(t, list):
        return [np.ascontiguousarray(p) for p, _ in t]
    return [np.ascontiguousarray(w) for w in t[0]]


def _cut(buf, off):
    return [buf[int(off[k]):int(off[k + 1])].tobytes() for k in range(off.shape[0] - 1)]


def _check_call(ens, tracers, rows, encoders, decoder, done):
    """One raw call: bytes_out, offsets, step, and every world's stream against its own oracle encoder; the decoder follows."""
    buf, off, step = ens.h.deltas(tracers=tracers)
    assert step == done
    assert off.shape == (len(rows) + 1,) and off[0] == 0 and int(off[-1]) == buf.shape[0]
    assert not (off % 8).any()
    streams = _cut(buf, off)
    for k, (enc, now) in enumerate(zip(encoders, rows)):
        want = enc.encode(now, step=done)
        assert len(streams[k]) == len(want), (k, len(streams[k]), len(want))
        assert streams[k] == want, k
    decoder.apply(streams)
    assert decoder.step == done
    for k, got in enumerate(decoder.positions()):
        assert _same_bits(got, rows[k]), k
    return streams


CASES = [("ensemble", [65] * 5, None), ("ensemble", [4096] * 3, None), ("ensemble64", [65] * 5, None), ("ensemble64", [4096] * 3, None),
         ("restricted", [65] * 5, [130] * 5), ("restricted", [4096] * 3, [130] * 3),
         ("restricted64", [65] * 5, [130] * 5), ("restricted64", [4096] * 3, [130] * 3),
         ("ragged", RAGGED_SIZES, None), ("ragged64", RAGGED_SIZES, None),
         ("rr", RAGGED_SIZES, RAGGED_TRACERS), ("rr64", RAGGED_SIZES, RAGGED_TRACERS)]


@pytest.mark.parametrize("handle,sizes,tracers", CASES, ids=[f"{h}-{s[0]}x{len(s)}" for h, s, _ in CASES])
def test_every_worlds_stream_equals_the_format_statement_of_that_world_alone(nb, handle, sizes, tracers):
    dtype = np.float64 if handle.endswith("64") else np.float32
    ens = _make(nb, handle, sizes, tracers, dtype, seed=11)
    try:
        b = len(sizes)
        enc_b, enc_t = [dc.Encoder() for _ in range(b)], [dc.Encoder() for _ in range(b)]
        dec_b, dec_t = nb.DeltasDecoder(b), nb.DeltasDecoder(b)
        done = 0
        first = later = None
        for gap in GAPS:
            if gap:
                ens.update(0.1, n_steps=gap)
                done += gap
            streams = _check_call(ens, False, _body_rows(ens), enc_b, dec_b, done)     # the two sequences in alternation
            if tracers is not None:
                ts = _check_call(ens, True, _tracer_rows(ens), enc_t, dec_t, done)
                for k, m in enumerate(tracers):
                    if m == 0:
                        assert len(ts[k]) == 32                                       # an empty segment: its header alone
            first = first or streams
            later = streams
        assert all(s[5] == 1 for s in first) and all(s[5] == 0 for s in later)
        assert sum(map(len, later)) < sum(map(len, first))                            # deltas are smaller than key frames
    finally:
        ens.close()


@pytest.mark.parametrize("handle", ["restricted", "rr64"])
def test_tracer_streams_of_a_handle_that_holds_none_are_headers_of_no_rows(nb, handle):
    dtype = np.float64 if handle.endswith("64") else np.float32
    sizes = [65] * 3 if handle == "restricted" else [1, 64, 65]
    ens = _make(nb, handle, sizes, None, dtype, seed=3)
    try:
        streams, step = ens.deltas(tracers=True)
        assert step == 0 and len(streams) == 3
        empty = np.zeros((0, 2), dtype)
        for s in streams:
            assert s == dc.Encoder().encode(empty, step=0) and len(s) == 32
        bodies, _ = ens.deltas()
        for k, p in enumerate(_body_rows(ens)):
            assert bodies[k] == dc.Encoder().encode(p, step=0)
    finally:
        ens.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_worlds_bytes_do_not_depend_on_its_neighbours(nb, dtype):
    """World k of the ragged ensemble against an ensemble holding world k alone, stepped the same way under EXACT, and at step
    0 against a context holding that world's rows."""
    rng = np.random.default_rng(11)
    worlds = [_rows(n, dtype, rng, special=k == 1) for k, n in enumerate(RAGGED_SIZES)]
    cls = nb.RaggedEnsemble64 if dtype == np.float64 else nb.RaggedEnsemble
    full = cls([w[0] for w in worlds], [w[1] for w in worlds], arith="exact")
    alone = [cls([w[0]], [w[1]], arith="exact") for w in worlds]
    try:
        for gap in GAPS:
            if gap:
                full.update(0.1, n_steps=gap)
                for e in alone:
                    e.update(0.1, n_steps=gap)
            streams, step = full.deltas()
            for k, e in enumerate(alone):
                one, step1 = e.deltas()
                assert step1 == step and len(one) == 1
                assert one[0] == streams[k], (gap, k)
            if not gap:
                for k, (p, v) in enumerate(worlds):
                    world = nb.World(p, v, np.ones(len(p), np.uint32), method="direct")
                    try:
                        world.delta_begin()
                        stream, cstep = world.delta_end()
                    finally:
                        world.close()
                    assert cstep == 0 and stream == streams[k], k
    finally:
        full.close()
        for e in alone:
            e.close()


@pytest.mark.parametrize("arith", ["fast", "exact"])
@pytest.mark.parametrize("handle", ["rr", "rr64"])
def test_stepping_with_streams_in_between_gives_the_bits_of_stepping_alone(nb, handle, arith):
    dtype = np.float64 if handle.endswith("64") else np.float32
    a = _make(nb, handle, RAGGED_SIZES, RAGGED_TRACERS, dtype, seed=21, arith=arith, special_world=-1)
    b = _make(nb, handle, RAGGED_SIZES, RAGGED_TRACERS, dtype, seed=21, arith=arith, special_world=-1)
    try:
        for _ in range(4):
            a.deltas()
            a.deltas(tracers=True)
            a.update(0.1)
            b.update(0.1)
        a.deltas(key=True)
        pa, va, _ = a.particles()
        pb, vb, _ = b.particles()
        for k in range(len(RAGGED_SIZES)):
            assert _same_bits(pa[k], pb[k]) and _same_bits(va[k], vb[k]), k
        for (tpa, tva), (tpb, tvb) in zip(a.tracers(), b.tracers()):
            assert _same_bits(tpa, tpb) and _same_bits(tva, tvb)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("handle", ["ensemble", "rr64"])
def test_a_refused_call_changes_nothing(nb, handle):
    C = nb._capi
    dtype = np.float64 if handle.endswith("64") else np.float32
    sizes, tracers = ([65] * 5, None) if handle == "ensemble" else (RAGGED_SIZES, RAGGED_TRACERS)
    a = _make(nb, handle, sizes, tracers, dtype, seed=31)
    twin = _make(nb, handle, sizes, tracers, dtype, seed=31)
    try:
        for e in (a, twin):
            e.deltas()
            e.update(0.1)
        want, off, step = twin.h.deltas()
        with pytest.raises(C.NBodyError, match="smaller than the stream") as err:
            a.h.deltas(cap=64)
        assert err.value.needed == want.shape[0]
        with pytest.raises(C.NBodyError, match="smaller than the stream") as err:
            a.h.deltas(cap=0, key=True)                               # a question for the size; its key flag does not stick
        assert err.value.needed > want.shape[0]
        got, off2, step2 = a.h.deltas()
        assert step2 == step == 1 and np.array_equal(off, off2) and np.array_equal(got, want)
        assert all(s[5] == 0 for s in _cut(got, off2))
        a.update(0.1)
        twin.update(0.1)
        assert a.deltas() == twin.deltas()                            # and the sequence goes on as the twin's
    finally:
        a.close()
        twin.close()


def test_key_frames_on_demand_and_after_uploads(nb):
    dtype = np.float32
    sizes, counts = [65, 130, 1], [64, 0, 200]
    ens = _make(nb, "rr", sizes, counts, dtype, seed=41)
    try:
        flags = lambda streams: [s[5] for s in streams]
        assert flags(ens.deltas()[0]) == [1, 1, 1] and flags(ens.deltas(tracers=True)[0]) == [1, 1, 1]
        ens.update(0.1)
        assert flags(ens.deltas()[0]) == [0, 0, 0] and flags(ens.deltas(tracers=True)[0]) == [0, 0, 0]
        ens.update(0.1)
        streams, step = ens.deltas(key=True)                          # a key frame on demand: it decodes alone
        assert flags(streams) == [1, 1, 1] and step == 2
        dec = nb.DeltasDecoder(3)
        dec.apply(streams)
        for k, p in enumerate(_body_rows(ens)):
            assert _same_bits(dec.positions()[k], p)
            assert streams[k] == dc.Encoder().encode(p, step=2)
        assert flags(ens.deltas(tracers=True)[0]) == [0, 0, 0]        # the key flag addressed the bodies' sequence only
        # an upload of tracers: their next streams are key frames, the bodies' sequence goes on
        rng = np.random.default_rng(42)
        new = [_rows(m, dtype, rng) for m in (3, 70, 0)]
        ens.set_tracers(new)
        ens.update(0.1)
        ts, step = ens.deltas(tracers=True)
        assert flags(ts) == [1, 1, 1] and step == 3
        for k, p in enumerate(_tracer_rows(ens)):
            assert ts[k] == dc.Encoder().encode(p, step=3)
        bs, _ = ens.deltas()
        assert flags(bs) == [0, 0, 0]
        dec.apply(bs)
        for k, p in enumerate(_body_rows(ens)):
            assert _same_bits(dec.positions()[k], p)
        # an upload of bodies: both sequences start over, the step counts on
        worlds = [_rows(n, dtype, rng) for n in (2, 66)]
        ens.upload([w[0] for w in worlds], [w[1] for w in worlds], tracers=[None, _rows(5, dtype, rng)])
        bs, step = ens.deltas()
        ts, tstep = ens.deltas(tracers=True)
        assert flags(bs) == [1, 1] and flags(ts) == [1, 1] and step == tstep == 3
        for k, w in enumerate(worlds):
            assert bs[k] == dc.Encoder().encode(w[0], step=3)
        ens.update(0.1, n_steps=2)
        assert ens.deltas()[1] == 5 and flags(ens.deltas()[0]) == [0, 0]
    finally:
        ens.close()


HANDLE_CLASSES = {"ensemble": "EnsembleHandle", "ensemble64": "Ensemble64Handle", "ragged": "RaggedHandle", "ragged64": "Ragged64Handle",
                  "restricted": "RestrictedHandle", "restricted64": "Restricted64Handle", "rr": "RRHandle", "rr64": "RR64Handle"}


@pytest.mark.parametrize("handle", list(HANDLE_CLASSES))
def test_refusals_name_the_handle_and_leave_it_working(nb, handle):
    C = nb._capi
    word = WORDS[handle] + " deltas"
    dtype = np.float64 if handle.endswith("64") else np.float32
    h = getattr(C, HANDLE_CLASSES[handle])(0)
    raw = getattr(h.lib, "nbody_deltas_" + handle)
    try:
        with pytest.raises(C.NBodyError, match="nothing uploaded") as err:        # before an upload
            h.deltas()
        assert err.value.code == C.ERR_INVALID and word in str(err.value)
        assert h._call("_last_error").decode().startswith(word)
    finally:
        h.close()
    has_tracers = handle.startswith(("restricted", "rr"))
    sizes = [65, 65] if handle.rstrip("64") in ("ensemble", "restricted") else [65, 3]
    ens = _make(nb, handle, sizes, None, dtype, seed=51)
    try:
        h = ens.h
        out = np.full(1 << 16, 7, np.uint8)
        size, step = ctypes.c_size_t(77), ctypes.c_uint64(77)
        refused = [(4, C._ptr(out), out.size, ctypes.byref(size)), (0x80000000, C._ptr(out), out.size, ctypes.byref(size)),
                   (0, None, 8, ctypes.byref(size)), (0, C._ptr(out), out.size, None)]
        if not has_tracers:
            refused.append((C.DELTAS_TRACERS, C._ptr(out), out.size, ctypes.byref(size)))
        for flags, p, cap, bytes_out in refused:
            assert raw(h.h, flags, p, cap, bytes_out, None, ctypes.byref(step)) == C.ERR_INVALID, flags
            assert h._call("_last_error").decode().startswith(word), h._call("_last_error")
        assert (out == 7).all() and size.value == 77 and step.value == 77
        if not has_tracers:
            with pytest.raises(TypeError):
                ens.deltas(tracers=True)                                          # the class takes no such argument
        # the handle works afterwards, and its first stream is still the key frame
        streams, step = ens.deltas()
        for k, p in enumerate(_body_rows(ens)):
            assert streams[k] == dc.Encoder().encode(p, step=0)
    finally:
        ens.close()


def test_more_than_2_24_blocks_are_refused_naming_the_limit(nb):
    C = nb._capi
    b = (1 << 24) + 1
    pos = np.zeros((b, 1, 2), np.float32)
    h = C.EnsembleHandle(0)
    try:
        h.upload(b, 1, pos, pos, None)
        with pytest.raises(C.NBodyError, match=r"2\^24 blocks") as err:
            h.deltas()
        assert err.value.code == C.ERR_INVALID and "ensemble deltas" in str(err.value)
        assert h.shape == (b, 1)
    finally:
        h.close()
