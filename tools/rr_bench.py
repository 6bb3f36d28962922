#!/usr/bin/env python3
"""Ragged restricted ensemble against what the library offered before it: the same worlds and tracers, the same steps, the same
GPU, the same process.

    python tools/rr_bench.py [--out FILE] [--shapes 256:64-2048:256-16384] [--steps 20] [--reps 3] [--leg-timeout 240]
                             [--dtype f32|f64]

A shape B:lo-hi:mlo-mhi is B worlds whose sizes are drawn uniformly from lo .. hi and whose tracer counts are drawn uniformly
from mlo .. mhi (seeded).  For every shape and for FAST and EXACT arithmetic one LEG runs once, in a child process of its own
under its own time limit (a leg that fails or runs out of time is reported as such; after one that died or hung nothing more is
started):
  one handle   nb.RaggedRestrictedEnsemble of the B worlds, one call update(delta, n_steps=steps);
  per shape    one nb.RestrictedEnsemble per distinct (n, m), holding the worlds of that shape, created and uploaded beforehand,
               each stepped with update(delta, n_steps=steps) in turn.
Both are warmed up by one call, then timed `reps` times alternately with the host clock around the whole call — every call ends
in a synchronise of its stream.  The pair rate is steps * sum (n_k^2 + m_k n_k) pairs per call at 14 flop per pair,
against the 157.3 TFLOP/s f32 peak: an end-to-end figure of the call, launches and synchronise included, not a kernel's.
--dtype f64 measures nb.RaggedRestrictedEnsemble64 against one nb.RestrictedEnsemble64 per distinct (n, m), the rate against the
78.6 TFLOP/s f64 vector peak; FAST is then the opt-in arithmetic, EXACT the default chain.
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
    b, rng, trng = shape.split(":")
    lo, hi = (int(v) for v in rng.split("-"))
    mlo, mhi = (int(v) for v in trng.split("-"))
    return int(b), lo, hi, mlo, mhi


def leg(shape, arith, steps, reps, f64=False):
    import numpy as np
    import nbody_simulation_amd as nb
    b, lo, hi, mlo, mhi = parse_shape(shape)
    real = np.float64 if f64 else np.float32
    ragged_cls, uniform_cls = ((nb.RaggedRestrictedEnsemble64, nb.RestrictedEnsemble64) if f64 else
                               (nb.RaggedRestrictedEnsemble, nb.RestrictedEnsemble))
    rng = np.random.default_rng(0x7A66ED)
    sizes = rng.integers(lo, hi + 1, b).tolist()
    counts = rng.integers(mlo, mhi + 1, b).tolist()
    worlds = [nb.scenes.plummer(n, seed=0xE5E0000 + k) for k, n in enumerate(sizes)]
    pos = [np.ascontiguousarray(w[0], real) for w in worlds]
    vel = [np.ascontiguousarray(w[1], real) for w in worlds]
    wgt = [w[2] for w in worlds]
    tracers = []
    for k, m in enumerate(counts):   # tracers scattered over their world's extent, at rest relative to its centre
        c, s = pos[k].mean(axis=0), pos[k].std(axis=0) + 1.0
        tracers.append((np.ascontiguousarray(c + s * rng.normal(0, 1, (m, 2)), real), np.zeros((m, 2), real)))
    one = ragged_cls(pos, vel, wgt, tracers, arith=arith)
    groups = {}
    for k, nm in enumerate(zip(sizes, counts)):
        groups.setdefault(nm, []).append(k)
    per_shape = [uniform_cls(np.stack([pos[k] for k in ks]), np.stack([vel[k] for k in ks]), np.stack([wgt[k] for k in ks]),
                             (np.stack([tracers[k][0] for k in ks]), np.stack([tracers[k][1] for k in ks])), arith=arith)
                 for _, ks in sorted(groups.items())]
    bplan, tplan = nb.ragged_plan(sizes, dtype=real), nb.rr_plan(sizes, counts, dtype=real)

    def run_one():
        t = time.perf_counter()
        one.update(0.1, None, n_steps=steps)
        return time.perf_counter() - t

    def run_per_shape():
        t = time.perf_counter()
        for e in per_shape:
            e.update(0.1, None, n_steps=steps)
        return time.perf_counter() - t

    run_one(), run_per_shape()            # warm-up: code objects
    t1, tp = [], []
    for _ in range(reps):
        t1.append(run_one())
        tp.append(run_per_shape())
    # both sides have taken the same steps of the same worlds: FAST and EXACT agree bit for bit between them
    rp, _, _ = one.particles()
    rt = one.tracers()
    same = True
    for e, (_, ks) in zip(per_shape, sorted(groups.items())):
        ep, _, _ = e.particles()
        etp, etv = e.tracers()
        same = same and all(ep[i].tobytes() == rp[k].tobytes() and etp[i].tobytes() == rt[k][0].tobytes() and
                            etv[i].tobytes() == rt[k][1].tobytes() for i, k in enumerate(ks))
        e.close()
    one.close()
    return dict(shape=shape, arith=arith, steps=steps, worlds=b, rows=int(sum(sizes)), tracer_rows=int(sum(counts)),
                pairs=int(sum(n * n + m * n for n, m in zip(sizes, counts))), distinct=len(groups),
                launches=len(bplan["blocks"]) + len(tplan["blocks"]), blocks=int(bplan["blocks"].sum() + tplan["blocks"].sum()),
                same_bits=bool(same), one_s=t1, per_shape_s=tp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--shapes", default="256:64-2048:256-16384")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--leg-timeout", type=float, default=240.0)
    ap.add_argument("--dtype", choices=("f32", "f64"), default="f32")
    ap.add_argument("--leg", help=argparse.SUPPRESS)   # SHAPE/arith — the child process of one leg
    a = ap.parse_args()
    if a.leg:
        shape, arith = a.leg.split("/")
        print("LEG " + json.dumps(leg(shape, arith, a.steps, a.reps, f64=a.dtype == "f64")), flush=True)
        return 0
    if not os.path.exists("/dev/kfd"):
        print("rr_bench: no GPU here; a measurement path does not fall back", file=sys.stderr)
        return 2
    f64 = a.dtype == "f64"
    peak = PEAK_F64 if f64 else PEAK_F32
    lines = [f"# tools/rr_bench.py{' --dtype f64' if f64 else ''}: steps per call {a.steps}, timed calls per side {a.reps} (alternating, after one warm-up call each)",
             "# shape B:lo-hi:mlo-mhi = B worlds, sizes drawn uniformly from lo .. hi, tracer counts from mlo .. mhi (seeded);",
             f"# per shape = one nb.RestrictedEnsemble{'64' if f64 else ''} per distinct (n, m), each update() in turn",
             "# seconds are host-clock times of one whole call (it ends in a stream synchronise); ratio = per shape / one handle (medians)",
             f"# rate = steps * sum (n_k^2 + m_k n_k) pairs per call * {FLOP_PER_PAIR} flop over the median time of the one handle, as a share of "
             f"{peak / 1e12:.1f} TFLOP/s (end to end)",
             f"{'shape':>24} {'arith':>6} {'one_handle_s (each call)':>28} {'per_shape_s (each call)':>28} {'ratio':>7} {'TFLOP/s':>8} {'of peak':>8}   plan"]
    for shape in a.shapes.split(","):
        for arith in ("fast", "exact"):
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", f"{shape}/{arith}", "--steps", str(a.steps), "--reps", str(a.reps)] + (["--dtype", "f64"] if f64 else [])
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout)
            except subprocess.TimeoutExpired:
                lines.append(f"{shape:>24} {arith:>6}  leg ran out of its {a.leg_timeout:.0f} s")
                break    # a leg that hangs: nothing more is started on the device
            rec = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
            if r.returncode != 0 or not rec:
                lines.append(f"{shape:>24} {arith:>6}  leg failed (exit {r.returncode}): {r.stderr.strip().splitlines()[-1:] or ''}")
                if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
                    break
                continue
            d = json.loads(rec[0])
            t1, tp = sorted(d["one_s"]), sorted(d["per_shape_s"])
            m1, mp = t1[len(t1) // 2], tp[len(tp) // 2]
            flops = d["pairs"] * d["steps"] * FLOP_PER_PAIR / m1
            lines.append(f"{shape:>24} {arith:>6} {' '.join(f'{t:.5f}' for t in d['one_s']):>28} {' '.join(f'{t:.5f}' for t in d['per_shape_s']):>28} "
                         f"{mp / m1:7.2f} {flops / 1e12:8.2f} {100 * flops / peak:7.1f}%   {d['rows']} rows, {d['tracer_rows']} tracers, "
                         f"{d['distinct']} distinct (n, m), {d['launches']} launches of {d['blocks']} blocks per step, "
                         f"bits {'equal' if d['same_bits'] else 'DIFFER'}")
        else:
            continue
        break
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
