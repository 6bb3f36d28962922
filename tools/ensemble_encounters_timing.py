#!/usr/bin/env python3
"""Encounters of an ensemble against what a user did before them and against a force evaluation of the same pairs: the same
worlds, the same GPU, the same process.

    python tools/ensemble_encounters_timing.py [--out FILE] [--trials 5] [--calls 20]

Three shapes: the bodies of 256 worlds x 1 024 bodies in float32 (nb.Ensemble) and in float64 (nb.Ensemble64), and the tracers of
64 worlds x 1 024 bodies x 16 384 tracers (nb.RestrictedEnsemble, float32).  Every handle runs under arith="exact".  Per shape:
  encounters()     one call on the ensemble with all three per-row arrays: two launches, the copies to the host, a synchronise;
  records only     the same with rows=False: the records alone are copied back;
  download+host    what a user did before: particles() (or tracers()) and nb.encounters_of per world on the host — records and
                   rows are compared bit for bit with encounters()'s before anything is timed;
  accel()          one accel() (for the tracers: tracers_accel()) of the same handle: the same ordered pairs under the exact
                   pair law, two divisions each, and the copy of the accelerations to the host.
After one warm-up pass of everything, a TRIAL times each in turn: the host clock around `calls` calls of encounters(), of the
records only and of accel(), and around one pass of download + host (every call ends in a synchronise of the handle's stream).
Reported: the median over the trials of the seconds per call, and the least and the largest trial.  These are end-to-end times of
host calls; they are no kernel times.  There is no threshold in this file: it records.  This is a tool, not a test: it needs an
MI355X and fails without one.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H = 100_000
LIMIT2 = 1.0e4      # squared world units: some pairs of every world are close, most are not


def measure(dtype, worlds, n, m, trials, calls):
    import numpy as np
    import nbody_simulation_amd as nb
    rng = np.random.default_rng(0xE1C0 + n + m + np.dtype(dtype).itemsize)
    pos = rng.uniform(0.0, H, (worlds, n, 2)).astype(dtype)
    vel = rng.standard_normal((worlds, n, 2)).astype(dtype)
    w = rng.integers(1, 13, (worlds, n)).astype(np.uint32)
    limit2 = np.full(worlds, LIMIT2, np.float32)
    if m:
        tpos = rng.uniform(0.0, H, (worlds, m, 2)).astype(dtype)
        tvel = rng.standard_normal((worlds, m, 2)).astype(dtype)
        ens = nb.RestrictedEnsemble(pos, vel, w, (tpos, tvel), arith="exact")
    else:
        ens = (nb.Ensemble if dtype == np.float32 else nb.Ensemble64)(pos, vel, w, arith="exact")

    def encounters(rows=True):
        return ens.encounters(limit2, True, rows) if m else ens.encounters(limit2, rows)

    def host():
        p = ens.particles()[0]
        if m:
            t = ens.tracers()[0]
            return [nb.encounters_of(t[k], p[k], dtype(LIMIT2)) for k in range(worlds)]
        return [nb.encounters_of(p[k], None, dtype(LIMIT2)) for k in range(worlds)]

    def accel():
        return ens.tracers_accel() if m else ens.accel()

    ens.update(0.01)
    got, want = encounters(), host()               # warm-up of every way, and the bits
    same = all(got[0][k].tobytes() == want[k][0].tobytes() and all(got[i][k].tobytes() == want[k][i].tobytes() for i in (1, 2, 3))
               for k in range(worlds))
    same = same and encounters(False)[0].tobytes() == got[0].tobytes()
    accel()
    t = dict(encounters=[], records=[], host=[], accel=[])
    for _ in range(trials):
        for name, fn in (("encounters", encounters), ("records", lambda: encounters(False)), ("accel", accel)):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            t[name].append((time.perf_counter() - t0) / calls)
        t0 = time.perf_counter()
        host()
        t["host"].append(time.perf_counter() - t0)
    ens.close()
    return same, {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        print("ensemble_encounters_timing: no GPU here; a measurement path does not fall back", file=sys.stderr)
        return 2
    import numpy as np
    lines = [f"# tools/ensemble_encounters_timing.py: {a.trials} trials after one warm-up pass; a trial times {a.calls} calls of encounters(), {a.calls} of",
             f"# encounters(rows=False), {a.calls} of accel() (tracers: tracers_accel()) under arith=\"exact\", and one pass of download +",
             f"# nb.encounters_of per world on the host, in that order; limit2 = {LIMIT2:g} in every world",
             "# seconds per call, host clock around calls that end in a stream synchronise: median (least .. largest trial)",
             f"{'worlds x bodies x tracers':>28} {'dtype':>8} {'targets':>8} {'ordered pairs':>14} {'encounters()':>34} {'records only':>34} "
             f"{'download + host encounters_of':>34} {'one accel() under EXACT':>34} {'host/enc':>9} {'accel/enc':>10}  bits"]
    for dtype, worlds, n, m in ((np.float32, 256, 1024, 0), (np.float64, 256, 1024, 0), (np.float32, 64, 1024, 16384)):
        same, t = measure(dtype, worlds, n, m, a.trials, a.calls)

        def fmt(k):
            med, lo, hi = t[k]
            return f"{med * 1e3:9.3f} ms ({lo * 1e3:8.3f} .. {hi * 1e3:8.3f})"

        pairs = worlds * (m * n if m else n * (n - 1))
        lines.append(f"{f'{worlds} x {n} x {m}':>28} {np.dtype(dtype).name:>8} {'tracers' if m else 'bodies':>8} {pairs:>14} {fmt('encounters'):>34} "
                     f"{fmt('records'):>34} {fmt('host'):>34} {fmt('accel'):>34} {t['host'][0] / t['encounters'][0]:9.1f} "
                     f"{t['accel'][0] / t['encounters'][0]:10.2f}  {'equal' if same else 'DIFFER'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
