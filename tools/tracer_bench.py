"""What tracers cost in a direct step (product library; the headline bench is bench.py).  Writes a small text report:

  (a) N = M = 2^20 Plummer, f32 FAST: ms per step without and with 2^20 tracers; the difference is the tracer cost.
  (b) one nbody_accel_direct_at_f32 call of 2^20 targets over the same bodies — with this tree's library and, given
      --parent-lib PATH, with a library built from the parent commit, on the same device in the same run.  (a)'s tracer cost and
      (b) do the same pairs with the same main pass; (a) drops the host copies and the per-batch synchronisation.
  (c) the restricted reference scene (the 2 heavy bodies of galaxy(), the rest tracers) next to the whole scene as bodies.

Every figure is the median of 5 timed runs after a warm-up, host clock around calls that end in a stream synchronise.

    python tools/tracer_bench.py [--parent-lib PATH] [--out profiles/tracers_direct.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 1 << 20
RUNS = 5


def _median_ms(call, per=1):
    call()  # warm-up: allocations, code objects
    t = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3 / per)
    return float(np.median(t)), [round(x, 3) for x in t]


def _bodies_and_points(nb):
    pos, vel, w = nb.scenes.plummer(N, seed=0x1F1F)
    rng = np.random.default_rng(29)
    pts = (pos + rng.normal(0, 1, pos.shape)).astype(np.float32)
    return pos, vel, w, pts, rng.normal(0, 1, pos.shape).astype(np.float32)


def leg_b(lib_path):
    """In a process of its own, so that the library under test is the only one loaded."""
    import nbody_simulation_amd as nb
    C = nb._capi
    if lib_path:  # an older build: bind what it exports (it has the probe call; it may lack what came after)
        import ctypes
        C._share_hip_runtime_with_torch()
        have = ctypes.CDLL(lib_path)
        C._SIGS = {k: v for k, v in C._SIGS.items() if hasattr(have, k)}
        C.LIB_PATH = lib_path
    pos, vel, w, pts, _ = _bodies_and_points(nb)
    with C.Context(0) as ctx:
        ctx.set_params(arith=C.ARITH_FAST)
        ctx.upload(pos, vel, w)
        ms, runs = _median_ms(lambda: ctx.accel_direct(pts))
    print(json.dumps({"ms": ms, "runs": runs}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libnbody_hip.so built from the parent commit, for leg (b)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracers_direct.txt"))
    ap.add_argument("--leg-b", default=None, metavar="LIB", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg_b is not None:
        return leg_b(a.leg_b)
    import nbody_simulation_amd as nb
    C = nb._capi
    lines = ["tracers in a direct step: median of %d runs after a warm-up (tools/tracer_bench.py)" % RUNS, ""]
    pos, vel, w, pts, pvel = _bodies_and_points(nb)
    steps = 2
    with C.Context(0) as ctx:
        ctx.set_params(arith=C.ARITH_FAST)
        ctx.upload(pos, vel, w)
        plain, r0 = _median_ms(lambda: ctx.update_direct(0.1, steps), steps)
        ctx.upload(pos, vel, w)
        ctx.upload_tracers(pts, pvel)
        both, r1 = _median_ms(lambda: ctx.update_direct(0.1, steps), steps)
    cost = both - plain
    lines += ["(a) N = M = 2^20 Plummer, f32 FAST, ms per step",
              "    bodies alone        %9.3f   runs %s" % (plain, r0),
              "    bodies + tracers    %9.3f   runs %s" % (both, r1),
              "    tracer cost         %9.3f" % cost, ""]
    lines.append("(b) one nbody_accel_direct_at_f32 call, 2^20 targets over the same bodies, ms")
    b_ms = {}
    for name, path in (("this tree", ""), ("parent commit", a.parent_lib)):
        if path is None:
            lines.append("    %-19s not measured (no --parent-lib)" % name)
            continue
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg-b", os.path.abspath(path) if path else ""], check=True, capture_output=True, text=True)
        res = json.loads(out.stdout.strip().splitlines()[-1])
        b_ms[name] = res["ms"]
        lines.append("    %-19s %9.3f   runs %s" % (name, res["ms"], res["runs"]))
    ref = b_ms.get("parent commit", b_ms.get("this tree"))
    lines += ["    tracer cost (a) / call (b, %s) = %.3f  (expected: not above 1.02)" % ("parent commit" if "parent commit" in b_ms else "this tree",
                                                                                      cost / ref), ""]
    spos, svel, sw = nb.scenes.galaxy()
    (bp, bv, bw), (tp, tv) = nb.scenes.restricted(spos, svel, sw, 2)
    steps = 20
    with C.Context(0) as ctx:
        ctx.upload(spos, svel, sw)
        whole, r2 = _median_ms(lambda: ctx.update_direct(0.1, steps), steps)
        ctx.upload(bp, bv, bw)
        ctx.upload_tracers(tp, tv)
        restricted, r3 = _median_ms(lambda: ctx.update_direct(0.1, steps), steps)
    lines += ["(c) the reference scene (galaxy(), %d rows), f32 AUTO, ms per step" % len(spos),
              "    every row a body                  %9.3f   runs %s" % (whole, r2),
              "    2 bodies + %d tracers         %9.3f   runs %s" % (len(tp), restricted, r3), ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
