"""Wall time per step of nbody_update_direct_f32 at small N, where the host's work per step shows: the captured pair of steps
replayed (the default) and eager steps (NBODY_DIRECT_GRAPH=0).  One line per size and mode: the median and the spread of
`--repeats` timings of `--steps` steps each, after a warm-up call.  Product library.  Needs an MI355X.

    python tools/direct_small_n.py [--steps 2000] [--repeats 7]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    import nbody_simulation_amd as nb
    C = nb._capi
    for n in (1024, 16384):
        pos, vel, w = nb.scenes.plummer(n, seed=3)
        for graph in ("1", "0"):
            os.environ["NBODY_DIRECT_GRAPH"] = graph
            with C.Context(0) as ctx:
                ctx.upload(pos, vel, w)
                ctx.update_direct(0.1, 100)
                us = []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    ctx.update_direct(0.1, args.steps)          # returns after a stream synchronise
                    us.append((time.perf_counter() - t0) / args.steps * 1e6)
            print("n %6d  %-6s  median %8.2f us/step  min %8.2f  max %8.2f" %
                  (n, "graph" if graph == "1" else "eager", float(np.median(us)), min(us), max(us)), flush=True)


if __name__ == "__main__":
    main()
