"""Digests of the direct step of the bodies themselves: the sha256 of the final rows after a few steps, one line per case.

Run with two builds (say, a parent commit's and this tree's) on the same device, the outputs must be equal line for line when a
change claims to leave the bits alone — FAST included.  Cases, Plummer bodies, dt = 0.1, default (AUTO) arithmetic unless named:
  uniform / sparse / classes3   40 000 bodies, 3 steps: equal masses; one mass but for 20 heavy bodies; masses 1, 2, 3 — each with the
                                near/far split as the size decides (off) and forced (NBODY_DIRECT_NEARFAR=2)
  free                          70 001 bodies with free masses, 3 steps (the split engages by size)
  graph                         1 024 and 40 000 equal-mass bodies, 6 steps: the captured pair of steps replayed
  exact                         40 000 bodies, masses 1, 2, 3, EXACT arithmetic, 3 steps
  mutual / streamed             laboratory library, 16 384 equal-mass bodies, FAST, NBODY_DIRECT_MUTUAL_MIN_N=0 and the split forced, 3 steps;
                                then the same under NBODY_DIRECT_ASM=3 (no mutual pass: its digest differs)
  multi                         40 000 bodies, masses 1 .. 4, a two-chunk multi context that lists device 0 twice, 3 steps
Needs an MI355X.

    python tools/direct_digest.py [--out FILE]
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _setenv(**kw):
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import nbody_simulation_amd as nb
    C = nb._capi
    lines = []

    def case(name, make, pos, vel, w, steps, **params):
        with make() as c:
            if params:
                c.set_params(**params)
            c.upload(pos, vel, w)
            c.update_direct(0.1, steps)
            p, v, w2, ids = c.download()
        lines.append("%-28s n %6d  steps %d  rows %s" % (name, len(pos), steps, _sha(p, v, w2, ids)))
        print(lines[-1], flush=True)

    def single():
        return C.Context(0)

    n = 40_000
    pos, vel, ones = nb.scenes.plummer(n, seed=0xD16E58)
    heavy = ones.copy()
    heavy[::2000] = 750_000
    three = (np.arange(n) % 3 + 1).astype(np.uint32)
    for split in (None, "2"):
        _setenv(NBODY_DIRECT_NEARFAR=split)
        tag = " split forced" if split else ""
        case("uniform" + tag, single, pos, vel, ones, 3)
        case("sparse" + tag, single, pos, vel, heavy, 3)
        case("classes3" + tag, single, pos, vel, three, 3)
    _setenv(NBODY_DIRECT_NEARFAR=None)
    pf, vf, _ = nb.scenes.plummer(70_001, seed=0xD16E59)
    case("free", single, pf, vf, nb.scenes.free_weights(70_001), 3)
    case("graph", single, pos[:1024], vel[:1024], ones[:1024], 6)
    case("graph", single, pos, vel, ones, 6)
    case("exact", single, pos, vel, three, 3, arith=C.ARITH_EXACT)
    _setenv(NBODY_DIRECT_MUTUAL_MIN_N="0", NBODY_DIRECT_NEARFAR="2")
    with C.laboratory():
        case("mutual (lab)", single, pos[:16384], vel[:16384], ones[:16384], 3, arith=C.ARITH_FAST)
        _setenv(NBODY_DIRECT_ASM="3")  # the one-sided streamed pass: other bits, so the line above is the mutual pass's
        case("streamed (lab)", single, pos[:16384], vel[:16384], ones[:16384], 3, arith=C.ARITH_FAST)
        _setenv(NBODY_DIRECT_ASM=None)
    _setenv(NBODY_DIRECT_MUTUAL_MIN_N=None, NBODY_DIRECT_NEARFAR=None)
    case("multi [0, 0] two chunks", lambda: C.MultiContext([0, 0], C.EXCHANGE_PEER, 2), pos, vel, (np.arange(n) % 4 + 1).astype(np.uint32), 3)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
