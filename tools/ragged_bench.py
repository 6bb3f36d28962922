#!/usr/bin/env python3
"""Ragged ensemble against what the library offered before it: the same worlds, the same steps, the same GPU, the same process.

    python tools/ragged_bench.py [--out FILE] [--shapes 256:64-2048,4096:8-512,256:1024-1024] [--steps 20] [--reps 3] [--leg-timeout 240]
                                 [--dtype f32|f64]

A shape B:lo-hi is B worlds whose sizes are drawn uniformly from lo .. hi (seeded; lo == hi: equal sizes).  For every shape and
for FAST and EXACT arithmetic one LEG runs once, in a child process of its own under its own time limit (a leg that fails or
runs out of time is reported as such; after one that died or hung nothing more is started):
  ragged     nb.RaggedEnsemble of the B worlds, one call update(delta, n_steps=steps);
  per size   one nb.Ensemble per distinct size, holding the worlds of that size, created and uploaded beforehand, each stepped
             with update(delta, n_steps=steps) in turn (with equal sizes that is one nb.Ensemble: the uniform kernel).
Both are warmed up by one call, then timed `reps` times alternately with the host clock around the whole call — every call ends
in a synchronise of its stream.  The pair rate is steps * sum n_k^2 pairs per call at 14 flop per pair, against
the 157.3 TFLOP/s f32 peak: an end-to-end figure of the call, launches and synchronise included, not a kernel's.
--dtype f64 measures nb.RaggedEnsemble64 against one nb.Ensemble64 per distinct size, on float64 worlds; the rate is then a share
of the 78.6 TFLOP/s f64 vector peak (AMD's public figure for the part).
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


def parse_shape(shape):
    b, rng = shape.split(":")
    lo, hi = (int(v) for v in rng.split("-"))
    return int(b), lo, hi


def leg(shape, arith, steps, reps, dtype="f32"):
    import numpy as np
    import nbody_simulation_amd as nb
    b, lo, hi = parse_shape(shape)
    f64 = dtype == "f64"
    real = np.float64 if f64 else np.float32
    Ragged, Uniform = (nb.RaggedEnsemble64, nb.Ensemble64) if f64 else (nb.RaggedEnsemble, nb.Ensemble)
    sizes = np.random.default_rng(0x7A66ED).integers(lo, hi + 1, b).tolist()
    worlds = [nb.scenes.plummer(n, seed=0xE5E0000 + k, dtype=real) for k, n in enumerate(sizes)]
    pos = [np.ascontiguousarray(w[0], real) for w in worlds]
    vel = [np.ascontiguousarray(w[1], real) for w in worlds]
    wgt = [w[2] for w in worlds]
    rag = Ragged(pos, vel, wgt, arith=arith)
    groups = {}
    for k, n in enumerate(sizes):
        groups.setdefault(n, []).append(k)
    per_size = [Uniform(np.stack([pos[k] for k in ks]), np.stack([vel[k] for k in ks]), np.stack([wgt[k] for k in ks]), arith=arith)
                for _, ks in sorted(groups.items())]
    plan = nb.ragged_plan(sizes, dtype=real)

    def run_ragged():
        t = time.perf_counter()
        rag.update(0.1, None, n_steps=steps)
        return time.perf_counter() - t

    def run_per_size():
        t = time.perf_counter()
        for e in per_size:
            e.update(0.1, None, n_steps=steps)
        return time.perf_counter() - t

    run_ragged(), run_per_size()            # warm-up: code objects
    tr, tp = [], []
    for _ in range(reps):
        tr.append(run_ragged())
        tp.append(run_per_size())
    # both sides have taken the same steps of the same worlds: FAST and EXACT agree bit for bit between them
    rp, _, _ = rag.particles()
    same = True
    for e, (_, ks) in zip(per_size, sorted(groups.items())):
        ep, _, _ = e.particles()
        same = same and all(ep[i].tobytes() == rp[k].tobytes() for i, k in enumerate(ks))
        e.close()
    rag.close()
    return dict(shape=shape, arith=arith, steps=steps, worlds=b, rows=int(sum(sizes)), pairs=int(sum(n * n for n in sizes)),
                distinct=len(groups), launches=len(plan["blocks"]), blocks=int(plan["blocks"].sum()), same_bits=bool(same),
                ragged_s=tr, per_size_s=tp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--shapes", default="256:64-2048,4096:8-512,256:1024-1024")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--leg-timeout", type=float, default=240.0)
    ap.add_argument("--dtype", choices=("f32", "f64"), default="f32")
    ap.add_argument("--leg", help=argparse.SUPPRESS)   # SHAPE/arith — the child process of one leg
    a = ap.parse_args()
    f64 = a.dtype == "f64"
    peak = PEAK_F64 if f64 else PEAK_F32
    if a.leg:
        shape, arith = a.leg.split("/")
        print("LEG " + json.dumps(leg(shape, arith, a.steps, a.reps, a.dtype)), flush=True)
        return 0
    if not os.path.exists("/dev/kfd"):
        print("ragged_bench: no GPU here; a measurement path does not fall back", file=sys.stderr)
        return 2
    lines = [f"# tools/ragged_bench.py: steps per call {a.steps}, timed calls per side {a.reps} (alternating, after one warm-up call each)",
             "# shape B:lo-hi = B worlds, sizes drawn uniformly from lo .. hi (seeded); per size = one nb.Ensemble per distinct size, each update() in turn",
             "# seconds are host-clock times of one whole call (it ends in a stream synchronise); ratio = per size / ragged (medians)",
             f"# rate = steps * sum n_k^2 pairs per ragged call * {FLOP_PER_PAIR} flop over the median time, as a share of {peak / 1e12:.1f} TFLOP/s (end to end)",
             f"{'shape':>14} {'arith':>6} {'ragged_s (each call)':>28} {'per_size_s (each call)':>28} {'ratio':>7} {'TFLOP/s':>8} {'of peak':>8}   plan"]
    if f64:
        lines[0] = lines[0].replace("tools/ragged_bench.py:", "tools/ragged_bench.py --dtype f64 (nb.RaggedEnsemble64 against one nb.Ensemble64 per distinct size):")
        lines[1] = lines[1].replace("one nb.Ensemble per distinct size", "one nb.Ensemble64 per distinct size")
        lines.insert(4, "# the peak is the f64 vector peak, AMD's public figure")
    first = a.shapes.split(",")[0]
    worst = None
    for shape in a.shapes.split(","):
        for arith in ("fast", "exact"):
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", f"{shape}/{arith}", "--steps", str(a.steps), "--reps", str(a.reps), "--dtype", a.dtype]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout)
            except subprocess.TimeoutExpired:
                lines.append(f"{shape:>14} {arith:>6}  leg ran out of its {a.leg_timeout:.0f} s")
                break    # a leg that hangs: nothing more is started on the device
            rec = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
            if r.returncode != 0 or not rec:
                lines.append(f"{shape:>14} {arith:>6}  leg failed (exit {r.returncode}): {r.stderr.strip().splitlines()[-1:] or ''}")
                if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
                    break
                continue
            d = json.loads(rec[0])
            tr, tp = sorted(d["ragged_s"]), sorted(d["per_size_s"])
            mr, mp = tr[len(tr) // 2], tp[len(tp) // 2]
            flops = d["pairs"] * d["steps"] * FLOP_PER_PAIR / mr
            ratio = mp / mr
            if shape == first:
                worst = ratio if worst is None else min(worst, ratio)
            lines.append(f"{shape:>14} {arith:>6} {' '.join(f'{t:.5f}' for t in d['ragged_s']):>28} {' '.join(f'{t:.5f}' for t in d['per_size_s']):>28} "
                         f"{ratio:7.2f} {flops / 1e12:8.2f} {100 * flops / peak:7.1f}%   {d['rows']} rows, {d['distinct']} distinct sizes, "
                         f"{d['launches']} launches of {d['blocks']} blocks, bits {'equal' if d['same_bits'] else 'DIFFER'}")
        else:
            continue
        break
    if worst is not None:
        lines.append(f"# condition (first shape, both arithmetics): ragged no slower than the loop over per-size ensembles: "
                     f"{'met' if worst >= 1.0 else 'NOT met'} (lowest ratio {worst:.2f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
