#!/usr/bin/env python3
"""Ensemble against a loop over contexts: the same worlds, the same steps, the same GPU, the same process.

    python tools/ensemble_bench.py [--out FILE] [--shapes 256x1024,4096x256,64x4096] [--steps 20] [--reps 3] [--leg-timeout 240]
                                   [--dtype f32|f64]

For every shape B x n and for FAST and EXACT arithmetic one LEG runs once, in a child process of its own under its own time
limit (a leg that fails or runs out of time is reported as such and the others still run):
  ensemble   nb.Ensemble of the B worlds, one call update(delta, n_steps=steps);
  contexts   what the library offered before ensembles: one Context per world, created and uploaded beforehand, each stepped
             with update_direct(delta, steps) in turn.  At most 256 contexts are created; a shape with more worlds goes round
             them B / 256 times (the same number of calls on worlds of the same size).
Both are warmed up by one call, then timed `reps` times alternately with the host clock around the whole call — every call ends
in a synchronise of its stream.  The pair rate is B * n^2 * steps pairs per ensemble call at 14 flop per pair,
against the 157.3 TFLOP/s f32 peak: an end-to-end figure of the call, launches and synchronise included, not a kernel's.
--dtype f64 measures nb.Ensemble64 against the same yardstick in double: one f64 Context per world (float64 arrays uploaded),
each stepped with update_direct in turn; the f64 step is not replayed from a captured graph, so that loop pays its launches
every step.  The rate is then a share of the 78.6 TFLOP/s f64 vector peak (AMD's public figure for the part; the hardware
guide, MI355X_MICROARCH.md, has no f64 vector row), and the f32 ensemble of the same worlds and
arithmetic is timed in the same leg and quoted beside it.  The 240 s leg default holds for f64 too: the slowest leg is EXACT over
contexts — 64 x 4096 is 64 * 20 steps of ~16.8 M pairs on 16 blocks each, a fraction of a second per call, and 4096 x 256 is 82 k
small launches per call, seconds — times four calls (one warm-up, three timed).
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


def leg(b, n, arith, steps, reps, dtype="f32"):
    import numpy as np
    import nbody_simulation_amd as nb
    C = nb._capi
    f64 = dtype == "f64"
    worlds = [nb.scenes.plummer(n, seed=0xE5E0000 + k, dtype=np.float64 if f64 else np.float32) for k in range(b)]
    pos = np.stack([w[0] for w in worlds])
    vel = np.stack([w[1] for w in worlds])
    wgt = np.stack([w[2] for w in worlds])
    ens = (nb.Ensemble64 if f64 else nb.Ensemble)(pos, vel, wgt, arith=arith)
    ens32 = nb.Ensemble(pos.astype(np.float32), vel.astype(np.float32), wgt, arith=arith) if f64 else None
    nctx = min(b, MAX_CONTEXTS)
    rounds = (b + nctx - 1) // nctx
    ctxs = []
    for k in range(nctx):
        c = C.Context(0)
        c.set_params(arith={"fast": C.ARITH_FAST, "exact": C.ARITH_EXACT}[arith])
        c.upload(pos[k], vel[k], wgt[k])
        ctxs.append(c)

    def run_ensemble():
        t = time.perf_counter()
        ens.update(0.1, None, n_steps=steps)
        return time.perf_counter() - t

    def run_contexts():
        t = time.perf_counter()
        for _ in range(rounds):
            for c in ctxs:
                c.update_direct(0.1, steps)
        return time.perf_counter() - t

    def run_ensemble32():
        t = time.perf_counter()
        ens32.update(0.1, None, n_steps=steps)
        return time.perf_counter() - t

    run_ensemble(), run_contexts()           # warm-up: code objects, the contexts' captured graphs
    te, tc, t32 = [], [], []
    if ens32 is not None:
        run_ensemble32()
    for _ in range(reps):
        te.append(run_ensemble())
        tc.append(run_contexts())
        if ens32 is not None:
            t32.append(run_ensemble32())
    for c in ctxs:
        c.close()
    ens.close()
    out = dict(b=b, n=n, arith=arith, steps=steps, contexts=nctx, rounds=rounds, ensemble_s=te, contexts_s=tc)
    if ens32 is not None:
        ens32.close()
        out["ensemble_f32_s"] = t32
    return out


def _f32_beside(d, flops):
    t32 = sorted(d["ensemble_f32_s"])
    m32 = t32[len(t32) // 2]
    f32 = d["b"] * d["n"] ** 2 * d["steps"] * FLOP_PER_PAIR / m32
    return f" {flops / FLOP_PER_PAIR / 1e9:9.1f}   {m32:.5f} s {f32 / 1e12:.2f} TFLOP/s {100 * f32 / PEAK_F32:.1f}%"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--shapes", default="256x1024,4096x256,64x4096")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--leg-timeout", type=float, default=240.0)
    ap.add_argument("--dtype", choices=("f32", "f64"), default="f32")
    ap.add_argument("--leg", help=argparse.SUPPRESS)   # BxN:arith — the child process of one leg
    a = ap.parse_args()
    f64 = a.dtype == "f64"
    peak = PEAK_F64 if f64 else PEAK_F32
    if a.leg:
        shape, arith = a.leg.split(":")
        b, n = (int(v) for v in shape.split("x"))
        print("LEG " + json.dumps(leg(b, n, arith, a.steps, a.reps, a.dtype)), flush=True)
        return 0
    if not os.path.exists("/dev/kfd"):
        print("ensemble_bench: no GPU here; a measurement path does not fall back", file=sys.stderr)
        return 2
    lines = [f"# tools/ensemble_bench.py: steps per call {a.steps}, timed calls per side {a.reps} (alternating, after one warm-up call each)",
             "# seconds are host-clock times of one whole call (it ends in a stream synchronise); ratio = contexts / ensemble (medians)",
             f"# rate = B*n^2*steps pairs per ensemble call * {FLOP_PER_PAIR} flop over the median time, as a share of {peak / 1e12:.1f} TFLOP/s (end to end)",
             f"{'shape':>10} {'arith':>6} {'ensemble_s (each call)':>34} {'contexts_s (each call)':>34} {'ratio':>7} {'TFLOP/s':>8} {'of peak':>8}"]
    if f64:
        lines[0] = lines[0].replace("tools/ensemble_bench.py:", "tools/ensemble_bench.py --dtype f64 (nb.Ensemble64 against one f64 Context per world):")
        lines.insert(3, f"# the peak is the f64 vector peak, AMD's public figure; Gpairs/s = B*n^2*steps / median time; f32 ens = nb.Ensemble of the same "
                        f"worlds and arithmetic, timed in the same leg (median s, TFLOP/s, share of {PEAK_F32 / 1e12:.1f})")
        lines[-1] += f" {'Gpairs/s':>9}   f32 ens"
    worst = None
    for shape in a.shapes.split(","):
        for arith in ("fast", "exact"):
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", f"{shape}:{arith}", "--steps", str(a.steps), "--reps", str(a.reps)]
            if f64:
                cmd += ["--dtype", "f64"]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout)
            except subprocess.TimeoutExpired:
                lines.append(f"{shape:>10} {arith:>6}  leg ran out of its {a.leg_timeout:.0f} s")
                break    # a leg that hangs: nothing more is started on the device
            rec = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
            if r.returncode != 0 or not rec:
                lines.append(f"{shape:>10} {arith:>6}  leg failed (exit {r.returncode}): {r.stderr.strip().splitlines()[-1:] or ''}")
                if r.returncode < 0 or r.returncode in (134, 139):
                    break
                continue
            d = json.loads(rec[0])
            te, tc = sorted(d["ensemble_s"]), sorted(d["contexts_s"])
            me, mc = te[len(te) // 2], tc[len(tc) // 2]
            flops = d["b"] * d["n"] ** 2 * d["steps"] * FLOP_PER_PAIR / me
            ratio = mc / me
            if shape == a.shapes.split(",")[0]:
                worst = ratio if worst is None else min(worst, ratio)
            lines.append(f"{shape:>10} {arith:>6} {' '.join(f'{t:.5f}' for t in d['ensemble_s']):>34} {' '.join(f'{t:.5f}' for t in d['contexts_s']):>34} "
                         f"{ratio:7.2f} {flops / 1e12:8.2f} {100 * flops / peak:7.1f}%"
                         + (_f32_beside(d, flops) if f64 else "")
                         + (f"   ({d['contexts']} contexts x {d['rounds']} rounds)" if d["rounds"] > 1 else ""))
        else:
            continue
        break
    if worst is not None:
        lines.append(f"# condition (first shape, both arithmetics): ensemble no slower than the loop over contexts: {'met' if worst >= 1.0 else 'NOT met'} (lowest ratio {worst:.2f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
