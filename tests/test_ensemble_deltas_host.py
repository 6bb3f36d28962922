"""Delta streams of an ensemble (nbody_deltas_*, the classes' deltas(), nb.DeltasDecoder) without a GPU: the nine declared names
in both libraries and in the binding, no other name under the prefix, the ABI version, NULL-handle calls, nbody_deltas_bound
against nbody_delta_bound and the oracle's key frames, and the decoder of many worlds on streams of the oracle's encoder."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import delta_codec as dc

HANDLES = ("ensemble", "ensemble64", "ragged", "ragged64", "restricted", "restricted64", "rr", "rr64")
CALLS = ["nbody_deltas_" + s for s in HANDLES]
NAMES = CALLS + ["nbody_deltas_bound"]


def test_header_declares_the_deltas_calls_and_both_libraries_export_them(nb):
    C = nb._capi
    assert len(NAMES) == 9
    declared = C.declared_symbols()
    assert sorted(s for s in declared if s.startswith("nbody_deltas_")) == sorted(NAMES)      # these and no other
    assert sorted(s for s in C._SIGS if s.startswith("nbody_deltas_")) == sorted(NAMES)
    assert sorted(C._SIGS) == declared
    for path in (C.LIB_PATH, C.LAB_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in NAMES if not hasattr(lib, s)], path
    with open(C.HEADER_PATH) as f:
        head = f.read()
    assert int(re.search(r"#define\s+NBODY_ABI_VERSION\s+(\d+)", head).group(1)) == 3 == C.ABI_VERSION    # new symbols only
    assert "nbody_deltas" not in head                                       # declared in nbody_ensemble.h, which it includes
    with open(os.path.join(os.path.dirname(C.HEADER_PATH), "nbody_ensemble.h")) as f:
        ens = f.read()
    for name in CALLS:
        handle = "nbody_" + name[len("nbody_deltas_"):]
        assert re.search(rf"int\s+{name}\s*\(\s*{handle}\s*\*\s*e,\s*uint32_t\s+flags,\s*uint8_t\s*\*\s*out,\s*size_t\s+cap,\s*"
                         r"size_t\s*\*\s*bytes_out,\s*uint64_t\s*\*\s*offsets_out,\s*uint64_t\s*\*\s*step_out\s*\)\s*;", ens), name
        assert len(C._SIGS[name][1]) == 7
    assert re.search(r"size_t\s+nbody_deltas_bound\s*\(\s*int64_t\s+n_segments,\s*const\s+int64_t\s*\*\s*rows\s*(/\*.*?\*/)?\s*,\s*int\s+is_f64\s*\)\s*;", ens)
    assert re.search(r"#define\s+NBODY_DELTAS_TRACERS\s+1u", ens) and re.search(r"#define\s+NBODY_DELTAS_KEY\s+2u", ens)
    assert (C.DELTAS_TRACERS, C.DELTAS_KEY) == (1, 2)
    # the prefix is its own: none of the nine falls into a handle's closed set of names, the frames' or the context's streams'
    assert not [s for s in NAMES if s.startswith(("nbody_ensemble_", "nbody_ensemble64_", "nbody_ragged_", "nbody_ragged64_",
                                                  "nbody_restricted_", "nbody_restricted64_", "nbody_rr_", "nbody_rr64_",
                                                  "nbody_frames_", "nbody_delta_"))]
    assert "DeltasDecoder" in nb.__all__ and nb.DeltasDecoder is nb.ensemble.DeltasDecoder
    for cls in (nb.Ensemble, nb.Ensemble64, nb.RaggedEnsemble, nb.RaggedEnsemble64, nb.RestrictedEnsemble, nb.RestrictedEnsemble64,
                nb.RaggedRestrictedEnsemble, nb.RaggedRestrictedEnsemble64):
        assert callable(cls.deltas), cls


@pytest.mark.parametrize("which", ["product", "lab"])
def test_null_handle_calls(nb, which):
    C = nb._capi
    lib = C._load(which)
    out = np.full(256, 7, np.uint8)
    offsets = np.full(4, 7, np.uint64)
    size, step = ctypes.c_size_t(77), ctypes.c_uint64(77)
    for name in CALLS:
        for flags in (0, 1, 2, 3):
            assert getattr(lib, name)(None, flags, C._ptr(out), out.size, ctypes.byref(size), C._ptr(offsets), ctypes.byref(step)) \
                == C.ERR_INVALID, name
        assert getattr(lib, name)(None, 0, None, 0, None, None, None) == C.ERR_INVALID, name
    assert (out == 7).all() and (offsets == 7).all() and size.value == 77 and step.value == 77


SIZE_LISTS = ([1], [0], [63, 64, 65], [4096] * 3, [0, 5000, 0])


def _bound(C, rows, f64):
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    return int(C.load().nbody_deltas_bound(rows.shape[0], C._ptr(rows), 1 if f64 else 0))


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("rows", SIZE_LISTS)
def test_bound_is_the_sum_of_the_single_bounds_and_holds_the_oracles_key_frames(nb, rows, f64):
    C = nb._capi
    lib = C.load()
    bound = _bound(C, rows, f64)
    assert bound == sum(int(lib.nbody_delta_bound(n, 1 if f64 else 0)) for n in rows)
    # random bit patterns: every width is the element's size or close to it, the largest a key frame gets
    rng = np.random.default_rng(len(rows) * 2 + f64)
    U, F = (np.uint64, np.float64) if f64 else (np.uint32, np.float32)
    total = 0
    for n in rows:
        pos = rng.integers(0, np.iinfo(U).max, size=(n, 2), dtype=U, endpoint=True).view(F)
        total += len(dc.Encoder().encode(pos, step=1))
    assert total <= bound
    assert bound % 8 == 0


def test_bound_refuses_what_it_cannot_describe(nb):
    C = nb._capi
    lib = C.load()
    rows = np.array([5, 6], np.int64)
    assert lib.nbody_deltas_bound(2, None, 0) == 0
    assert lib.nbody_deltas_bound(-1, C._ptr(rows), 0) == 0
    assert _bound(C, [5, -1, 6], False) == 0 and _bound(C, [5, -1, 6], True) == 0
    assert lib.nbody_deltas_bound(0, C._ptr(rows), 0) == 0                       # no segment: no bytes
    limit = 1 << 24
    ones = np.ones(limit + 1, np.int64)                                          # one block each
    assert lib.nbody_deltas_bound(limit + 1, C._ptr(ones), 0) == 0
    assert lib.nbody_deltas_bound(limit, C._ptr(ones), 0) == limit * int(lib.nbody_delta_bound(1, 0))
    assert _bound(C, [(1 << 30) + 1], False) == 0 and _bound(C, [1 << 62], True) == 0      # one segment of more than 2^24 blocks


def _special(pos):
    """NaN, +-inf and -0.0 planted among the rows (as many as there is room for)."""
    vals = [np.nan, np.inf, -np.inf, -0.0]
    flat = pos.reshape(-1)
    for i, v in enumerate(vals[:flat.size]):
        flat[(i * 7) % flat.size] = v
    return pos


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


WORLD_SIZES = [1, 64, 65, 0]


def _oracle_sequences(dtype, seed):
    """Three snapshots of worlds of WORLD_SIZES rows -> (positions[snapshot][world], streams[snapshot][world])."""
    rng = np.random.default_rng(seed)
    encoders = [dc.Encoder() for _ in WORLD_SIZES]
    positions, streams = [], []
    base = [_special((rng.random((n, 2)) * 1e5).astype(dtype)) for n in WORLD_SIZES]
    vel = [rng.standard_normal((n, 2)).astype(dtype) for n in WORLD_SIZES]
    for t in range(3):
        now = [(p + dtype(t) * v).astype(dtype) for p, v in zip(base, vel)]
        positions.append(now)
        streams.append([e.encode(p, step=10 + t) for e, p in zip(encoders, now)])
    return positions, streams


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_deltas_decoder_returns_every_worlds_bits(nb, dtype):
    positions, streams = _oracle_sequences(dtype, 5)
    dec = nb.DeltasDecoder(len(WORLD_SIZES))
    assert len(dec) == len(WORLD_SIZES)
    for t in range(3):
        dec.apply(streams[t])
        assert dec.step == 10 + t
        got = dec.positions()
        assert len(got) == len(WORLD_SIZES)
        for k, n in enumerate(WORLD_SIZES):
            assert got[k].shape == (n, 2) and _same_bits(got[k], positions[t][k]), (t, k)
    assert len(streams[0][3]) == 32                                              # an empty world is its header alone
    dec.close()


def test_deltas_decoder_refuses_a_wrong_length_and_applies_nothing_of_a_list_with_a_corrupt_stream(nb):
    C = nb._capi
    positions, streams = _oracle_sequences(np.float32, 6)
    dec = nb.DeltasDecoder(len(WORLD_SIZES))
    with pytest.raises(ValueError, match="streams expected"):
        dec.apply(streams[0][:3])
    with pytest.raises(ValueError, match="streams expected"):
        dec.apply(streams[0] + [streams[0][0]])
    with pytest.raises(ValueError):
        nb.DeltasDecoder(0)
    dec.apply(streams[0])
    dec.apply(streams[1])
    for damage in ("magic", "size", "width", "count"):
        bad = bytearray(streams[2][2])
        if damage == "magic":
            bad[0] ^= 0xff
        elif damage == "size":
            bad = bad[:-8]
        elif damage == "width":
            bad[32] = (bad[32] & 128) | ((bad[32] & 127) + 1) % 33            # the widths no longer add up to the payload
        else:
            bad[8] ^= 1                                                        # another body count than the state's
        with pytest.raises(C.NBodyError, match="world 2"):
            dec.apply(streams[2][:2] + [bytes(bad)] + streams[2][3:])
        got = dec.positions()
        for k in range(len(WORLD_SIZES)):                                      # every decoder is where it was
            assert _same_bits(got[k], positions[1][k]), (damage, k)
        assert dec.step == 11
    dec.apply(streams[2])                                                      # and the sequence goes on
    for k in range(len(WORLD_SIZES)):
        assert _same_bits(dec.positions()[k], positions[2][k])
    assert dec.step == 12
