"""ms per step of the f64 direct step (nbody_update_direct_f64), EXACT and FAST, by HIP events (nbody_timer).

Every (N, arith) runs in a child process of its own under its own time limit; the first failure ends the sweep.  Bodies: the
seeded Plummer set in f64, uneven weights.  One line per case: ms/step, pairs/s and f64 pair-throughput.

  python tools/direct_f64_timing.py [--n 65536 262144 1048576] [--arith exact fast] [--warmup 1] [--steps 3] [--limit 300]
  NBODY_HIP_LIBRARY=lab NBODY_DIRECT64_TB=16 python tools/direct_f64_timing.py ...   (laboratory A/B of the EXACT term block)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(n, arith, warmup, steps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import nbody_simulation_amd as nb
    C = nb._capi
    pos, vel, _ = nb.scenes.plummer(n, seed=0xD64, dtype=np.float64)
    w = (np.arange(n) % 7 + 1).astype(np.uint32)
    with C.Context(0) as ctx:
        ctx.set_params(arith={"exact": C.ARITH_EXACT, "fast": C.ARITH_FAST}[arith])
        ctx.upload(pos, vel, w)
        t = C.Timer()
        ctx.set_timer(t)
        ctx.update_direct(0.1, warmup)
        t.read(reset=True)
        ctx.update_direct(0.1, steps)
        ms_step, launches = t.read(reset=True)  # (the mean per timed launch: one launch bracket per step)
        ctx.set_timer(None)
        t.close()
        p = ctx.download()[0]
    pairs = float(n) * float(n)
    print(json.dumps({"n": n, "arith": arith, "steps": steps, "launches": launches, "ms_per_step": round(ms_step, 4),
                      "pairs_per_s": pairs / (ms_step * 1e-3), "finite": bool(np.isfinite(p).all()),
                      "tb": os.environ.get("NBODY_DIRECT64_TB"), "lib": os.environ.get("NBODY_HIP_LIBRARY", "product")}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[65536, 262144, 1048576])
    ap.add_argument("--arith", nargs="+", default=["exact", "fast"])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds per case")
    ap.add_argument("--one", nargs=2, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        one(int(a.one[0]), a.one[1], a.warmup, a.steps)
        return 0
    for n in a.n:
        for arith in a.arith:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", str(n), arith, "--warmup", str(a.warmup),
                   "--steps", str(a.steps)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(json.dumps({"n": n, "arith": arith, "error": f"time limit {a.limit} s"}), flush=True)
                return 1
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line:
                print(json.dumps({"n": n, "arith": arith, "error": f"exit {r.returncode}", "stderr": r.stderr[-2000:]}), flush=True)
                return 1
            print(line[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
