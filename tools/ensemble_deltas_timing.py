#!/usr/bin/env python3
"""Delta streams of an ensemble against the ways a user had before them: the same worlds, the same GPU, the same process.

    python tools/ensemble_deltas_timing.py [--out FILE] [--trials 5] [--calls 20]

Three shapes: 256 worlds x 1 024 bodies in float32 (nb.Ensemble) and in float64 (nb.Ensemble64), the bodies' streams; and 64
worlds x 1 024 bodies x 16 384 tracers in float32 (nb.RestrictedEnsemble), the tracers' streams.  Every world is a compact Plummer
sphere of its own seed (nb.scenes.plummer, CLUSTER below), the tracers a wider sphere around it; arith is EXACT everywhere so that the ensemble
and the contexts walk the same trajectories and their streams can be compared byte for byte, which is done for the first four
streams before anything is timed.  Three ways to hand the positions of all worlds to the host after a step:
  deltas          one call of the handle's deltas() (nbody_deltas_*): one NBD1 stream per world;
  download        the handle's download() (download_tracers()) of the same rows, raw: positions AND velocities, as the call is;
  context loop    one nb._capi.Context per world, created and uploaded beforehand: delta_begin / delta_end (for the tracers
                  tracers_delta_begin / tracers_delta_end) of each in turn — what the library offered before.
After one warm-up pass of everything, a TRIAL is `calls` rounds of: one step of the ensemble and of every context (not timed),
then the host clock around each way in turn.  Every way ends in a synchronise of its stream.  Reported per way: the median over
the trials of the seconds per hand-off of ALL worlds, and the least and the largest trial.  These are end-to-end times of host
calls from Python, the allocation of the receiving numpy buffers and the device-to-host copies included; they are no kernel
times.  The sizes are those of the key frame (stream 1) and of stream 4, against the raw bytes of the positions.  There is no
threshold in this file: it records.  This is a tool, not a test: it needs an MI355X and fails without one.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DT = 0.1
# A compact cluster, so that the accelerations show in the positions from one step to the next (the default sphere of 1 024 bodies
# of weight 1 is all but force-free, and force-free motion in f32 advances by the same number of ulps every step: the linear
# predictor then leaves nothing to send).  The tracers are a wider sphere around the same centre.
CLUSTER = dict(scale=50.0, clip=450.0, centre=(500.0, 500.0))
HALO = dict(scale=100.0, clip=450.0, centre=(500.0, 500.0))


def measure(worlds, n, m, dtype, trials, calls):
    import numpy as np
    import nbody_simulation_amd as nb
    C = nb._capi
    scenes = [nb.scenes.plummer(n, seed=0xD17A0000 + k, dtype=dtype, **CLUSTER) for k in range(worlds)]
    pos, vel, w = (np.stack([s[i] for s in scenes]) for i in range(3))
    tr = m > 0
    if tr:
        tscenes = [nb.scenes.plummer(m, seed=0x7AACE000 + k, dtype=dtype, **HALO) for k in range(worlds)]
        tpos, tvel = (np.stack([s[i] for s in tscenes]) for i in range(2))
        ens = nb.RestrictedEnsemble(pos, vel, w, (tpos, tvel), arith="exact")
    else:
        ens = (nb.Ensemble64 if dtype == np.float64 else nb.Ensemble)(pos, vel, w, arith="exact")
    singles = []
    for k in range(worlds):
        c = C.Context(0)
        c.set_params(arith=C.ARITH_EXACT)
        c.upload(pos[k], vel[k], w[k])
        if tr:
            c.upload_tracers(tpos[k], tvel[k])
        singles.append(c)

    def step():
        ens.update(DT)
        for c in singles:
            c.update_direct(DT, 1)

    def deltas():
        return ens.h.deltas(tracers=tr)

    def download():
        return ens.h.download_tracers() if tr else ens.h.download()

    def loop():
        out = []
        for c in singles:
            if tr:
                c.tracers_delta_begin()
                out.append(c.tracers_delta_end()[0])
            else:
                c.delta_begin()
                out.append(c.delta_end()[0])
        return out

    # the first four streams: the bytes compared, the sizes kept (this is the warm-up of every way, too)
    same, sizes = True, []
    for i in range(4):
        if i:
            step()
        buf, off, _ = deltas()
        ref = loop()
        download()
        same = same and all(buf[int(off[k]):int(off[k + 1])].tobytes() == ref[k] for k in range(worlds))
        sizes.append(int(buf.shape[0]))
    raw = worlds * (m if tr else n) * 2 * np.dtype(dtype).itemsize
    t = dict(deltas=[], download=[], loop=[])
    for _ in range(trials):
        acc = dict(deltas=0.0, download=0.0, loop=0.0)
        for _ in range(calls):
            step()
            for name, f in (("deltas", deltas), ("download", download), ("loop", loop)):
                t0 = time.perf_counter()
                f()
                acc[name] += time.perf_counter() - t0
        for name in acc:
            t[name].append(acc[name] / calls)
    for c in singles:
        c.close()
    ens.close()
    return same, raw, sizes, {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in t.items()}


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        print("ensemble_deltas_timing: no GPU here; a measurement path does not fall back", file=sys.stderr)
        return 2
    lines = [f"# tools/ensemble_deltas_timing.py: {a.trials} trials after a warm-up pass of four streams; a trial is {a.calls} rounds of one step of everything",
             "# (not timed), then one deltas() of the ensemble, one download() of the same rows, one pass of delta_begin / delta_end over one",
             "# Context per world, each under the host clock",
             "# seconds per hand-off of ALL worlds, host calls from Python that end in a stream synchronise: median (least .. largest trial)",
             "# bytes: raw = the positions alone (download() also copies the velocities); key = stream 1, all worlds; 4th = stream 4, all worlds",
             f"{'worlds x bodies x tracers':>28} {'dtype':>8} {'rows':>8} {'deltas()':>34} {'download()':>34} {'Context loop':>34} {'loop/deltas':>12} "
             f"{'raw B':>10} {'key B':>10} {'4th B':>10} {'4th B/row':>10}  streams"]
    for worlds, n, m, dtype in ((256, 1024, 0, np.float32), (256, 1024, 0, np.float64), (64, 1024, 16384, np.float32)):
        t_shape = time.perf_counter()
        same, raw, sizes, t = measure(worlds, n, m, dtype, a.trials, a.calls)
        print(f"ensemble_deltas_timing: {worlds} x {n} x {m} {np.dtype(dtype).name} took {time.perf_counter() - t_shape:.1f} s", file=sys.stderr, flush=True)

        def fmt(k):
            med, lo, hi = t[k]
            return f"{med * 1e3:9.3f} ms ({lo * 1e3:8.3f} .. {hi * 1e3:8.3f})"

        rows = worlds * (m if m else n)
        lines.append(f"{f'{worlds} x {n} x {m}':>28} {np.dtype(dtype).name:>8} {'tracers' if m else 'bodies':>8} {fmt('deltas'):>34} {fmt('download'):>34} "
                     f"{fmt('loop'):>34} {t['loop'][0] / t['deltas'][0]:12.1f} {raw:10d} {sizes[0]:10d} {sizes[3]:10d} {sizes[3] / rows:10.2f}  "
                     f"{'equal' if same else 'DIFFER'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
