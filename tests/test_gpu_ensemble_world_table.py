"""A ragged restricted handle's table of row ranges across uploads: summary() and encounters() after the tracers, and then the
bodies, have been replaced on a handle whose table was already built.  The table (every world's body and tracer rows, the first
summary chunk of its tracers, the first encounter tile of its bodies and of its tracers) is built by the first frames, summary
or encounters call after an upload and must be rebuilt after the next one.  Every record and every per-target row is compared
bit for bit with nb.summary_of / nb.encounters_of of that world's own rows.  Needs an MI355X.

Shapes.  Bodies 5, 257, 64 with tracers 0, 4097, 300; then tracers 256, 0, 4096 — a world gains tracers and another loses them,
a segment shrinks from two summary chunks (4097) to one (4096), and a segment's last encounter tile goes from partial to exactly
full (256 targets); then bodies 64, 5, 257 without tracers."""
import numpy as np
import pytest

import _encounters_restatement as ER
import _encounters_scene as ES
import _summary_restatement as SR
import _summary_scene as SS

pytestmark = pytest.mark.gpu
H = SS.HEIGHT
SIZES, COUNTS = [5, 257, 64], [0, 4097, 300]
NEW_COUNTS = [256, 0, 4096]
NEW_SIZES = [64, 5, 257]
LIMITS = ES.limits(3)


def _check(nb, ens, worlds, tracers, what, summary_first=True):
    """summary() and encounters() of the handle's bodies or tracers, called in that order or the other, against the oracles of
    `worlds`, the rows it holds."""
    dtype = worlds[0]["pos"].dtype.type
    if summary_first:
        summ = ens.summary(H, None, tracers)
    rec, idx, d2, close = ens.encounters(LIMITS, tracers)
    if not summary_first:
        summ = ens.summary(H, None, tracers)
    assert rec.shape == summ.shape == (len(worlds),)
    for k, x in enumerate(worlds):
        rows = (x["tpos"], x["tvel"], None) if tracers else (x["pos"], x["vel"], x["w"])
        want = nb.summary_of(*rows, None, H)
        assert SR.same(summ[k], want), f"{what}, tracers {tracers}, world {k}: summary differs in {SR.diff(summ[k], want)}"
        want = nb.encounters_of(x["tpos"], x["pos"], dtype(LIMITS[k])) if tracers else nb.encounters_of(x["pos"], None, dtype(LIMITS[k]))
        got = (rec[k], idx[k], d2[k], close[k])
        assert ER.same_segment(got, want), f"{what}, tracers {tracers}, world {k}: encounters differ in {ER.diff(got, want)}"


def _tracers(worlds):
    return [(x["tpos"], x["tvel"]) if len(x["tpos"]) else None for x in worlds]


@pytest.mark.parametrize("cls_name, dtype", [("RaggedRestrictedEnsemble", np.float32), ("RaggedRestrictedEnsemble64", np.float64)])
def test_summary_and_encounters_follow_new_tracers_and_new_bodies_on_a_handle_whose_table_was_built(nb, cls_name, dtype):
    worlds = SS.scene(SIZES, COUNTS, dtype)
    with getattr(nb, cls_name)([x["pos"] for x in worlds], [x["vel"] for x in worlds], [x["w"] for x in worlds], _tracers(worlds)) as ens:
        # stage 1: the table is built by frames, then read by the tracers' calls and the bodies'
        assert ens.frames(H, 100, tracers=True).shape == (3, 100, 100, 4)
        _check(nb, ens, worlds, True, "as uploaded")
        _check(nb, ens, worlds, False, "as uploaded")

        # stage 2: other tracers under the same bodies; encounters before summary, with and without tracers
        fresh = SS.scene(SIZES, NEW_COUNTS, dtype)
        worlds = [dict(x, tpos=y["tpos"], tvel=y["tvel"]) for x, y in zip(worlds, fresh)]
        ens.set_tracers(_tracers(worlds))
        _check(nb, ens, worlds, True, "after set_tracers", summary_first=False)
        _check(nb, ens, worlds, False, "after set_tracers", summary_first=False)
        assert ens.sizes == (SIZES, NEW_COUNTS)

        # stage 3: other bodies, no tracers
        worlds = SS.scene(NEW_SIZES, [0, 0, 0], dtype)
        ens.upload([x["pos"] for x in worlds], [x["vel"] for x in worlds], [x["w"] for x in worlds])
        _check(nb, ens, worlds, False, "after upload")
        assert ens.sizes == (NEW_SIZES, [0, 0, 0])
