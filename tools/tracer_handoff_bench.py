"""What the tracers cost on their way out of the device (product library; the headline bench is bench.py).  The reference scene
(galaxy()) twice: every row a body, and the restricted problem — its 2 heavy bodies with the other rows as tracers.  Writes a small
text report:

  (a) frame() of the scene as bodies next to frame(tracers=True) of the restricted scene: the same number of splats, in one launch
      and in two.  1250 x 1250, median of 9 calls after a warm-up, host clock around a call that ends in a stream synchronise (the
      frame's 6.25 MB copy to the host included in both).
  (b) the size of one tracer delta stream per direct step of the restricted scene, next to the raw positions.

    python tools/tracer_handoff_bench.py [--out profiles/tracers_handoff.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RUNS = 9


def _median_ms(call):
    call()  # warm-up: allocations, code objects
    t = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), [round(x, 3) for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracers_handoff.txt"))
    a = ap.parse_args()
    import nbody_simulation_amd as nb
    pos, vel, w = nb.scenes.galaxy()
    (bp, bv, bw), (tp, tv) = nb.scenes.restricted(pos, vel, w, 2)
    lines = ["tracers in the hand-off: the reference scene, %d rows, f32 (tools/tracer_handoff_bench.py)" % len(pos), ""]
    whole = nb.World(pos, vel, w, method="direct")
    restricted = nb.World(bp, bv, bw, method="direct", tracers=(tp, tv))
    try:
        for wd in (whole, restricted):
            wd.update(0.1)
        rows = [("frame(), %d bodies" % len(pos), lambda: whole.frame()),
                ("frame(tracers=True), 2 bodies + %d tracers" % len(tp), lambda: restricted.frame(tracers=True)),
                ("frame(), the 2 bodies alone", lambda: restricted.frame())]
        lines.append("(a) 1250 x 1250 frame, ms per call: median of %d after a warm-up" % RUNS)
        for name, call in rows:
            ms, runs = _median_ms(call)
            lines.append("    %-48s %8.3f   runs %s" % (name, ms, runs))
        sizes = []
        for _ in range(11):
            restricted.tracers_delta_begin()
            sizes.append(len(restricted.tracers_delta_end()[0]))
            restricted.update(0.1)
        raw = 8 * len(tp)
        lines += ["", "(b) tracer delta stream, one per direct step (0.1), bytes; raw positions: %d" % raw,
                  "    key frame   %9d   (%.3f of raw)" % (sizes[0], sizes[0] / raw),
                  "    deltas      %s" % sizes[1:],
                  "    mean delta  %9.0f   (%.3f of raw, %.2f B per tracer)" % (np.mean(sizes[2:]), np.mean(sizes[2:]) / raw,
                                                                               np.mean(sizes[2:]) / len(tp)), ""]
    finally:
        whole.close()
        restricted.close()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
