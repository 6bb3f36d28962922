"""Frames of an ensemble (nbody_frames_*, the classes' frames(), nb.contact_sheet) without a GPU: the eight declared names in
both libraries and in the binding, no other name under the prefix, the ABI version, NULL-handle calls, and the contact sheet —
pure numpy — tile by tile."""
import ctypes
import os
import re

import numpy as np
import pytest

NAMES = ["nbody_frames_" + s for s in ("ensemble", "ensemble64", "ragged", "ragged64", "restricted", "restricted64", "rr", "rr64")]
WITH_TRACERS = {"nbody_frames_restricted", "nbody_frames_restricted64", "nbody_frames_rr", "nbody_frames_rr64"}


def test_header_declares_the_frames_calls_and_both_libraries_export_them(nb):
    C = nb._capi
    assert len(NAMES) == 8
    declared = C.declared_symbols()
    assert sorted(s for s in declared if s.startswith("nbody_frames_")) == sorted(NAMES)      # these and no other
    assert sorted(s for s in C._SIGS if s.startswith("nbody_frames_")) == sorted(NAMES)
    assert sorted(C._SIGS) == declared
    for path in (C.LIB_PATH, C.LAB_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [s for s in NAMES if not hasattr(lib, s)], path
    with open(C.HEADER_PATH) as f:
        head = f.read()
    assert int(re.search(r"#define\s+NBODY_ABI_VERSION\s+(\d+)", head).group(1)) == 3 == C.ABI_VERSION    # new symbols only
    assert "nbody_frames" not in head                                       # declared in nbody_ensemble.h, which it includes
    with open(os.path.join(os.path.dirname(C.HEADER_PATH), "nbody_ensemble.h")) as f:
        ens = f.read()
    for name in NAMES:
        handle = "nbody_" + name[len("nbody_frames_"):]
        tracers = r"int\s+with_tracers,\s*" if name in WITH_TRACERS else ""
        assert re.search(rf"int\s+{name}\s*\(\s*{handle}\s*\*\s*e,\s*uint32_t\s+height,\s*uint32_t\s+render_px,\s*{tracers}uint8_t\s*\*\s*rgba_out\s*\)\s*;",
                         ens), name
        assert len(C._SIGS[name][1]) == (5 if name in WITH_TRACERS else 4)
    # the prefix is its own: none of the eight falls into a handle's closed set of names
    assert not [s for s in NAMES if s.startswith(("nbody_ensemble_", "nbody_ensemble64_", "nbody_ragged_", "nbody_ragged64_",
                                                  "nbody_restricted_", "nbody_restricted64_", "nbody_rr_", "nbody_rr64_"))]
    # frames are offered now; snapshots and delta streams of an ensemble still are not
    assert "delta streams and frames" not in ens and "snapshots and delta streams" in ens
    assert "contact_sheet" in nb.__all__ and nb.contact_sheet is nb.ensemble.contact_sheet
    for cls in (nb.Ensemble, nb.Ensemble64, nb.RaggedEnsemble, nb.RaggedEnsemble64, nb.RestrictedEnsemble, nb.RestrictedEnsemble64,
                nb.RaggedRestrictedEnsemble, nb.RaggedRestrictedEnsemble64):
        assert callable(cls.frames), cls


@pytest.mark.parametrize("which", ["product", "lab"])
def test_null_handle_calls(nb, which):
    C = nb._capi
    lib = C._load(which)
    out = np.full(4 * 4 * 4, 7, np.uint8)
    for name in NAMES:
        args = (100, 4, 1) if name in WITH_TRACERS else (100, 4)
        assert getattr(lib, name)(None, *args, C._ptr(out)) == C.ERR_INVALID, name
        assert getattr(lib, name)(None, *args, None) == C.ERR_INVALID, name
    assert (out == 7).all()


def _tiles(w, px):
    """Frames whose every pixel names its world, its place in the tile and its channel: a misplaced tile changes bytes."""
    f = np.zeros((w, px, px, 4), np.uint8)
    for k in range(w):
        f[k, :, :, 0] = k + 1
        f[k, :, :, 1] = np.arange(px)[:, None] + 1
        f[k, :, :, 2] = np.arange(px)[None, :] + 1
        f[k, :, :, 3] = 255 - k
    return f


@pytest.mark.parametrize("w", [1, 5, 9])
@pytest.mark.parametrize("cols", [None, 1, 2, 3, 4, 9, 12])
def test_contact_sheet_puts_every_tile_at_its_place(nb, w, cols):
    px = 3
    f = _tiles(w, px)
    keep = f.copy()
    sheet = nb.contact_sheet(f) if cols is None else nb.contact_sheet(f, cols=cols)
    c = {1: 1, 5: 3, 9: 3}[w] if cols is None else cols                     # ceil(sqrt(W))
    r = -(-w // c)
    assert sheet.dtype == np.uint8 and sheet.shape == (r * px, c * px, 4)
    for slot in range(r * c):
        tile = sheet[(slot // c) * px:(slot // c + 1) * px, (slot % c) * px:(slot % c + 1) * px]
        if slot < w:
            assert np.array_equal(tile, f[slot]), slot
        else:
            assert not tile.any(), slot                                     # the padding stays zero
    assert np.array_equal(f, keep)
    assert np.array_equal(nb.contact_sheet(f, c), sheet)                    # cols is positional too


def test_contact_sheet_refuses_what_is_no_stack_of_square_tiles(nb):
    for bad in (np.zeros((3, 3, 4), np.uint8), np.zeros((2, 3, 4, 4), np.uint8), np.zeros((0, 3, 3, 4), np.uint8)):
        with pytest.raises(ValueError, match="contact_sheet"):
            nb.contact_sheet(bad)
    with pytest.raises(ValueError, match="cols"):
        nb.contact_sheet(np.zeros((2, 3, 3, 4), np.uint8), cols=0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("height", [100_000, 800])
def test_the_oracle_draws_every_planted_row_as_the_scene_says(orc, dtype, height):
    """tests/_frames_scene.py on the CPU: the yardstick of the GPU tests sees what each planted row is there for."""
    import _frames_scene as S
    worlds = S.scene([600, 600, S.N_PLANTED - 1], [300, S.M_PLANTED, 300], dtype, height)
    G = (0, 255, 0, 255)
    for k in (0, 1):
        a = S.draw_world(orc, worlds[k], height, 100, tracers=False)
        b = S.draw_world(orc, worlds[k], height, 100, tracers=True)
        for f in (a, b):
            assert [int(f[S.ROW, c, 3]) for c in (10, 12, 14)] == [240, 250, 250]
            assert all(tuple(f[S.ROW, c, :3]) == (255, f[S.ROW, c, 1], f[S.ROW, c, 1]) for c in (10, 12, 14))
            assert tuple(f[S.ROW, 20]) == G and tuple(f[S.ROW, 22]) == G          # heavy before, heavy after
            assert tuple(f[S.ROW, 31]) == G and tuple(f[S.ROW, 42]) == G          # weight 11; a tracer on a heavy pixel
            assert f[S.ROW, 30, 0] == 255 and f[S.ROW, 30, 3] == 10               # weight 10 is light
            assert tuple(f[S.ROW, 35]) == (255, 255 - 0x10 - 10, 255 - 0x10 - 10, 20)     # the LATER row's v, not the larger
            assert [int(f[S.ROW, c, 1]) for c in (50, 51, 52, 53, 54)] == [0, 239, 0, 0, 255 - 0x10 - 238]
            assert [int(f[S.ROW, c, 3]) for c in (50, 51, 52, 53, 54)] == [10] * 5
            assert not f[S.ROW + 1].any()                                         # nothing random in the planted band
            assert f[99, 99].any() and f[0, 0].any()                              # nextafter(height, 0) and -0.0 are inside
        assert a[S.ROW, 40, 3] == 10 and b[S.ROW, 40, 3] == 20
        assert tuple(b[S.ROW, 40, :3]) == (255, 255 - 0x10 - 70, 255 - 0x10 - 70) != tuple(a[S.ROW, 40, :3])   # the tracer colours it
        assert not a[S.ROW, 44].any() and tuple(b[S.ROW, 44]) == (255, 239, 239, 10)   # -inf + NaN is NaN: 0 as u8
    # the worlds share their positions and differ in everything else
    assert np.array_equal(worlds[0]["pos"], worlds[1]["pos"], equal_nan=True)
    assert not np.array_equal(S.draw_world(orc, worlds[0], height, 100, False), S.draw_world(orc, worlds[1], height, 100, False))
    assert len(worlds[2]["pos"]) == S.N_PLANTED - 1 and not S.draw_world(orc, worlds[2], height, 100, False)[S.ROW].any()
