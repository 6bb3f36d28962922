"""Digests of the direct sum at points that are not bodies: the probe call and three tracer steps, product library.

Run with two builds (say, a parent commit's and this tree's) on the same device, the outputs must be equal line for line when a
change claims to leave the bits alone — FAST included.  Cases: f32 fast / auto / exact and f64 fast / exact, each over
  plummer    65 537 Plummer bodies with free masses, 70 000 targets near them
  reference  the reference scene (galaxy()), 70 000 targets near its bodies
with some targets exactly on bodies and some outside FAST's domain (the per-target EXACT route).  One line per case: the sha256
of the probe call's accelerations, and of the tracers' and the bodies' rows after three steps of dt = 0.1.  Needs an MI355X.

    python tools/targets_digest.py [--out FILE]
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = 70_000


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import nbody_simulation_amd as nb
    C = nb._capi
    arith_of = {"fast": C.ARITH_FAST, "auto": C.ARITH_AUTO, "exact": C.ARITH_EXACT}
    lines = []
    with C.Context(0) as ctx:
        for dt, ariths in ((np.float32, ("fast", "auto", "exact")), (np.float64, ("fast", "exact"))):
            for scene in ("plummer", "reference"):
                if scene == "plummer":
                    pos, vel, _ = nb.scenes.plummer(65_537, seed=0xD16E57, dtype=dt)
                    w = nb.scenes.free_weights(65_537)
                else:
                    pos, vel, w = nb.scenes.galaxy(dtype=dt)
                    pos, vel = pos.astype(dt), vel.astype(dt)
                rng = np.random.default_rng(0xD16)
                tgt = (pos[rng.integers(0, len(pos), M)] + rng.normal(0, 5, (M, 2))).astype(dt)
                tgt[::1000] = pos[rng.integers(0, len(pos), len(tgt[::1000]))]  # on bodies
                tgt[500::7000, 0] = 1e-30 if dt == np.float32 else 1e-305        # outside FAST's domain
                tvel = rng.normal(0, 1, (M, 2)).astype(dt)
                for arith in ariths:
                    ctx.set_params(arith=arith_of[arith])
                    ctx.upload(pos, vel, w)
                    acc = ctx.accel_direct(tgt)
                    ctx.upload_tracers(tgt, tvel)
                    ctx.update_direct(0.1, 3)
                    tp, tv = ctx.download_tracers()
                    bp, bv, _, _ = ctx.download()
                    lines.append("%s %-9s %-5s  probe %s  tracers %s  bodies %s" %
                                 (np.dtype(dt).name, scene, arith, _sha(acc), _sha(tp, tv), _sha(bp, bv)))
                    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
