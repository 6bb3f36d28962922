#!/usr/bin/env python3
"""Restricted ensemble against a loop over contexts with tracers: the same worlds, the same steps, the same GPU, the same process.

    python tools/restricted_bench.py [--out FILE] [--shapes 256x2x4096,256x64x4096,64x1024x16384] [--steps 20] [--reps 3]
                                     [--leg-timeout 240] [--dtype f32|f64]

For every shape B x n x m (worlds x bodies x tracers per world) and for FAST and EXACT arithmetic one LEG runs once, in a child
process of its own under its own time limit (a leg that fails or runs out of time is reported as such and the others still run):
  restricted  nb.RestrictedEnsemble of the B worlds with their tracers, one call update(delta, n_steps=steps);
  contexts    what the library offered before: one Context per world with its tracers (upload_tracers), created and uploaded
              beforehand, each stepped with update_direct(delta, steps) in turn.  At most 256 contexts are created; a shape with
              more worlds goes round them B / 256 times (the same number of calls on worlds of the same shape).
Both are warmed up by one call, then timed `reps` times alternately with the host clock around the whole call — every call ends
in a synchronise of its stream (the method of tools/ensemble_bench.py).  `spread` is the loop's own slowest minus
fastest timed call; the condition per leg is that the restricted call beats the loop's median by more than that.  The pair rate
is B * (n^2 + m*n) * steps pairs per restricted call — all body-body and tracer-body pairs — at 14 flop per pair
against the 157.3 TFLOP/s f32 peak: an end-to-end figure of the call, launches and synchronise included, not a kernel's.
--dtype f64 measures nb.RestrictedEnsemble64 against f64 contexts with f64 tracers, the rate against the 78.6 TFLOP/s f64 vector
peak (AMD's public figure for the part); the default, f32, is the measurement described above.
This is a tool, not a test: it needs an MI355X and fails without one.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_F32 = 157.3e12
PEAK_F64 = 78.6e12    # vector f64, AMD's public figure
FLOP_PER_PAIR = 14
MAX_CONTEXTS = 256


def leg(b, n, m, arith, steps, reps, f64=False):
    import numpy as np
    import nbody_simulation_amd as nb
    C = nb._capi
    dt = np.float64 if f64 else np.float32
    worlds = [nb.scenes.plummer(n, seed=0xE5E0000 + k, dtype=dt) for k in range(b)]
    pos = np.stack([w[0] for w in worlds]).astype(dt)
    vel = np.stack([w[1] for w in worlds]).astype(dt)
    wgt = np.stack([w[2] for w in worlds])
    rng = np.random.default_rng(0x7ACE)
    lo, hi = pos.min(axis=1, keepdims=True), pos.max(axis=1, keepdims=True)
    if n == 1:
        lo, hi = lo - 100.0, hi + 100.0
    tp = (lo + (hi - lo) * rng.random((b, m, 2))).astype(dt)   # tracers over their world's box
    tv = rng.normal(0, 1, (b, m, 2)).astype(dt)
    rst = (nb.RestrictedEnsemble64 if f64 else nb.RestrictedEnsemble)(pos, vel, wgt, (tp, tv), arith=arith)
    nctx = min(b, MAX_CONTEXTS)
    rounds = (b + nctx - 1) // nctx
    ctxs = []
    for k in range(nctx):
        c = C.Context(0)
        c.set_params(arith={"fast": C.ARITH_FAST, "exact": C.ARITH_EXACT}[arith])
        c.upload(pos[k], vel[k], wgt[k])
        c.upload_tracers(tp[k], tv[k])
        ctxs.append(c)

    def run_restricted():
        t = time.perf_counter()
        rst.update(0.1, None, n_steps=steps)
        return time.perf_counter() - t

    def run_contexts():
        t = time.perf_counter()
        for _ in range(rounds):
            for c in ctxs:
                c.update_direct(0.1, steps)
        return time.perf_counter() - t

    run_restricted(), run_contexts()          # warm-up: code objects, the contexts' workspaces
    tr, tc = [], []
    for _ in range(reps):
        tr.append(run_restricted())
        tc.append(run_contexts())
    for c in ctxs:
        c.close()
    rst.close()
    return dict(b=b, n=n, m=m, arith=arith, dtype="f64" if f64 else "f32", steps=steps, contexts=nctx, rounds=rounds, restricted_s=tr,
                contexts_s=tc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--shapes", default="256x2x4096,256x64x4096,64x1024x16384")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--leg-timeout", type=float, default=240.0)
    ap.add_argument("--dtype", choices=("f32", "f64"), default="f32")
    ap.add_argument("--leg", help=argparse.SUPPRESS)   # BxNxM:arith — the child process of one leg
    a = ap.parse_args()
    if a.leg:
        shape, arith = a.leg.split(":")
        b, n, m = (int(v) for v in shape.split("x"))
        print("LEG " + json.dumps(leg(b, n, m, arith, a.steps, a.reps, f64=a.dtype == "f64")), flush=True)
        return 0
    if not os.path.exists("/dev/kfd"):
        print("restricted_bench: no GPU here; a measurement path does not fall back", file=sys.stderr)
        return 2
    peak = PEAK_F64 if a.dtype == "f64" else PEAK_F32
    lines = [f"# tools/restricted_bench.py{' --dtype f64' if a.dtype == 'f64' else ''}: steps per call {a.steps}, timed calls per side {a.reps} (alternating, after one warm-up call each)",
             "# shape = worlds x bodies x tracers per world; seconds are host-clock times of one whole call (it ends in a stream synchronise)",
             "# ratio = contexts / restricted (medians); spread = the loop's slowest - fastest timed call; gain = contexts median - restricted median",
             f"# rate = B*(n^2 + m*n)*steps pairs per restricted call * {FLOP_PER_PAIR} flop over the median time, as a share of {peak / 1e12:.1f} TFLOP/s (end to end)",
             f"{'shape':>14} {'arith':>6} {'restricted_s (each call)':>34} {'contexts_s (each call)':>34} {'ratio':>7} {'gain_s':>9} {'spread_s':>9} {'TFLOP/s':>8} {'of peak':>8}"]
    missed = []
    for shape in a.shapes.split(","):
        for arith in ("fast", "exact"):
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", f"{shape}:{arith}", "--steps", str(a.steps), "--reps", str(a.reps),
                   "--dtype", a.dtype]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout)
            except subprocess.TimeoutExpired:
                lines.append(f"{shape:>14} {arith:>6}  leg ran out of its {a.leg_timeout:.0f} s")
                missed.append(f"{shape} {arith} (no result)")
                break    # a leg that hangs: nothing more is started on the device
            rec = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
            if r.returncode != 0 or not rec:
                missed.append(f"{shape} {arith} (no result)")
                lines.append(f"{shape:>14} {arith:>6}  leg failed (exit {r.returncode}): {r.stderr.strip().splitlines()[-1:] or ''}")
                if r.returncode < 0 or r.returncode in (134, 139):
                    break
                continue
            d = json.loads(rec[0])
            tr, tc = sorted(d["restricted_s"]), sorted(d["contexts_s"])
            mr, mc = tr[len(tr) // 2], tc[len(tc) // 2]
            spread = tc[-1] - tc[0]
            flops = d["b"] * (d["n"] ** 2 + d["m"] * d["n"]) * d["steps"] * FLOP_PER_PAIR / mr
            if not mc - mr > spread:
                missed.append(f"{shape} {arith}")
            lines.append(f"{shape:>14} {arith:>6} {' '.join(f'{t:.5f}' for t in d['restricted_s']):>34} {' '.join(f'{t:.5f}' for t in d['contexts_s']):>34} "
                         f"{mc / mr:7.2f} {mc - mr:9.5f} {spread:9.5f} {flops / 1e12:8.2f} {100 * flops / peak:7.1f}%"
                         + (f"   ({d['contexts']} contexts x {d['rounds']} rounds)" if d["rounds"] > 1 else ""))
        else:
            continue
        break
    lines.append("# condition (every leg): the restricted call is faster than the loop over contexts by more than the loop's own spread: "
                 + ("met" if not missed else "NOT met for " + ", ".join(missed)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
