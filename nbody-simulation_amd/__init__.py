"""nbody-simulation_amd — MI355X (gfx950) engine for the force + integration step of
KristinnVikarJ/nbody-simulation (reference: src/main.rs World::update, :388-425).

The product is the C-ABI shared library `lib/libnbody_hip.so` (include/nbody_hip.h) built from csrc/.
This Python package is the host-side mirror used by the tests and bench.py: a ctypes binding of that ABI
(`_capi`), `World`/`Counting` with the reference's names and call shape (`world`), `Ensemble` / `Ensemble64` — many small
worlds stepped together in one launch, in f32 / f64, and `RaggedEnsemble` / `RaggedEnsemble64` for worlds of different sizes, `RestrictedEnsemble` / `RestrictedEnsemble64` for worlds with tracers, `RaggedRestrictedEnsemble` / `RaggedRestrictedEnsemble64` for worlds of different sizes with tracers of their own, each with `frames()`, every world's draw() raster from one call, and `contact_sheet` to tile them, and with `deltas()`, every world's NBD1 delta stream from one call, which `DeltasDecoder` follows, and with `summary()`, a record per world of its moments, extent and separations, which `summary_of` restates on the host, and with `encounters()`, every body's or tracer's nearest neighbour and the pairs the clamp altered, which `encounters_of` restates on the host, and with `watch()` and `watch_sweep()`, a run or a sweep sampled on the device while it steps (`ensemble`) —, the seeded initial conditions (`scenes`) and the one-process-per-GPU sharded stepper (`sharding`).

Importable as `nbody_simulation_amd` (the repo root holds a symlink; a hyphen is not a Python identifier).
There is no CPU fallback: every compute entry point raises if the HIP library or a gfx950 device is missing.
"""
from . import _capi  # noqa: F401
from .world import Counting, World  # noqa: F401
from .ensemble import Ensemble, Ensemble64, RaggedEnsemble, RaggedEnsemble64, RestrictedEnsemble, RestrictedEnsemble64, RaggedRestrictedEnsemble, RaggedRestrictedEnsemble64, DeltasDecoder, contact_sheet, ragged_plan, rr_plan, resident_plan, summary_of, SUMMARY_DTYPE, encounters_of, ENCOUNTERS_DTYPE, watch_merge, watch_sweep_plan, WATCH_DTYPE, WATCH_NEVER  # noqa: F401
from ._capi import DeltaDecoder  # noqa: F401
from . import scenes  # noqa: F401

__all__ = ["World", "Counting", "Ensemble", "Ensemble64", "RaggedEnsemble", "RaggedEnsemble64", "RestrictedEnsemble", "RestrictedEnsemble64", "RaggedRestrictedEnsemble", "RaggedRestrictedEnsemble64", "ragged_plan", "rr_plan", "resident_plan", "contact_sheet", "DeltaDecoder", "DeltasDecoder", "summary_of", "SUMMARY_DTYPE", "encounters_of", "ENCOUNTERS_DTYPE", "watch_merge", "watch_sweep_plan", "WATCH_DTYPE", "WATCH_NEVER", "scenes", "_capi"]
