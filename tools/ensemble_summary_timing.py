#!/usr/bin/env python3
"""Summaries of an ensemble against what a user did before them and against a step: the same worlds, the same GPU, the same process.

    python tools/ensemble_summary_timing.py [--out FILE] [--trials 7] [--calls 100]

Three shapes: the bodies of 256 worlds x 1 024 bodies in float32 (nb.Ensemble) and in float64 (nb.Ensemble64), and the tracers of
64 worlds x 1 024 bodies x 16 384 tracers (nb.RestrictedEnsemble, float32; four chunks per world, so the second launch runs).
Each with world k measured from world k - 1 (ref), which is what a convergence or a seed study asks for.  Per shape:
  summary()        one call on the ensemble: the launches, the copy of the records to the host, a stream synchronise;
  download+host    what a user did before: particles() (or tracers()) and nb.summary_of per world on the host — the records
                   are compared bit for bit with summary()'s before anything is timed;
  update           one step of the same handle (update(delta), default arithmetic), for scale.
After one warm-up pass of everything, a TRIAL times each in turn: the host clock around `calls` calls of summary(), around one
pass of download + host, and around `calls` single-step updates (the summary is taken of the state those steps leave; every call
ends in a synchronise of the handle's stream).  Reported: the median over the trials of the seconds per call, and the least and
the largest trial.  These are end-to-end times of host calls; they are no kernel times.  There is no threshold in this file: it
records.  This is a tool, not a test: it needs an MI355X and fails without one.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H = 100_000


def same_records(np, a, b):
    for name in a.dtype.names:
        u, v = a[name], b[name]
        if u.dtype.kind == "f":
            nan = np.isnan(u) & np.isnan(v)
            if not np.array_equal(np.where(nan, 0, u.view(np.int64)), np.where(nan, 0, v.view(np.int64))):
                return False
        elif not np.array_equal(u, v):
            return False
    return True


def measure(dtype, worlds, n, m, trials, calls):
    import numpy as np
    import nbody_simulation_amd as nb
    rng = np.random.default_rng(0x5E77A + n + m + np.dtype(dtype).itemsize)
    pos = rng.uniform(0.0, H, (worlds, n, 2)).astype(dtype)
    vel = rng.standard_normal((worlds, n, 2)).astype(dtype)
    w = rng.integers(1, 13, (worlds, n)).astype(np.uint32)
    ref = (np.arange(worlds, dtype=np.int32) - 1) % worlds
    if m:
        tpos = rng.uniform(0.0, H, (worlds, m, 2)).astype(dtype)
        tvel = rng.standard_normal((worlds, m, 2)).astype(dtype)
        ens = nb.RestrictedEnsemble(pos, vel, w, (tpos, tvel))
    else:
        ens = (nb.Ensemble if dtype == np.float32 else nb.Ensemble64)(pos, vel, w)

    def summary():
        return ens.summary(H, ref, True) if m else ens.summary(H, ref)

    def host():
        if m:
            p, v = ens.tracers()
            return np.stack([nb.summary_of(p[k], v[k], None, (p[ref[k]], v[ref[k]]), H) for k in range(worlds)])
        p, v, ww = ens.particles()
        return np.stack([nb.summary_of(p[k], v[k], ww[k], (p[ref[k]], v[ref[k]]), H) for k in range(worlds)])

    ens.update(0.01)
    same = same_records(np, summary(), host())     # warm-up of every way, and the bits
    for _ in range(3):
        summary()
    t = dict(summary=[], host=[], update=[])
    for _ in range(trials):
        t0 = time.perf_counter()
        for _ in range(calls):
            summary()
        t["summary"].append((time.perf_counter() - t0) / calls)
        t0 = time.perf_counter()
        host()
        t["host"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for _ in range(calls):
            ens.update(0.01)
        t["update"].append((time.perf_counter() - t0) / calls)
    ens.close()
    return same, {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    a = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        print("ensemble_summary_timing: no GPU here; a measurement path does not fall back", file=sys.stderr)
        return 2
    import numpy as np
    lines = [f"# tools/ensemble_summary_timing.py: {a.trials} trials after one warm-up pass; a trial times {a.calls} calls of summary(), one pass of",
             f"# download + nb.summary_of per world on the host, and {a.calls} single-step update() calls, in that order; ref[k] = k - 1",
             "# seconds per call, host clock around calls that end in a stream synchronise: median (least .. largest trial)",
             f"{'worlds x bodies x tracers':>28} {'dtype':>8} {'segment':>8} {'summary()':>34} {'download + host summary_of':>34} {'one update() step':>34} "
             f"{'host/summary':>13} {'update/summary':>15}  records"]
    for dtype, worlds, n, m in ((np.float32, 256, 1024, 0), (np.float64, 256, 1024, 0), (np.float32, 64, 1024, 16384)):
        same, t = measure(dtype, worlds, n, m, a.trials, a.calls)

        def fmt(k):
            med, lo, hi = t[k]
            return f"{med * 1e3:9.3f} ms ({lo * 1e3:8.3f} .. {hi * 1e3:8.3f})"

        lines.append(f"{f'{worlds} x {n} x {m}':>28} {np.dtype(dtype).name:>8} {'tracers' if m else 'bodies':>8} {fmt('summary'):>34} {fmt('host'):>34} "
                     f"{fmt('update'):>34} {t['host'][0] / t['summary'][0]:13.1f} {t['update'][0] / t['summary'][0]:15.2f}  {'equal' if same else 'DIFFER'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
