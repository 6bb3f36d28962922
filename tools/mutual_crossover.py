"""Where the mutual main pass (csrc/direct_mutual.hip) starts to pay: the timed main pass of one equal-mass direct step through
nbody_direct_run_dev, direct_stream (lab NBODY_DIRECT_ASM=3) against the mutual pass (=4 with its lower bound lifted), over a
range of sizes.  Dev tool (laboratory build), not part of the product; results in profiles/r06_mutual_crossover.txt."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("NBODY_HIP_LIBRARY", "lab")  # the laboratory build honours NBODY_DIRECT_ASM / NBODY_DIRECT_MUTUAL_MIN_N
import nbody_simulation_amd as nb  # noqa: E402

C = nb._capi


def time_step(n, env, reps=3):
    import torch
    dev = torch.device("cuda:0")
    for k, v in env.items():
        os.environ[k] = str(v)
    pos, vel, w = nb.scenes.plummer(n, seed=1)
    tp = torch.from_numpy(pos).to(dev)
    tm = torch.from_numpy(w.astype(np.float32)).to(dev)
    tv = torch.from_numpy(vel.copy()).to(dev)
    out = torch.empty((n, 2), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    ws_bytes = C.direct_workspace_bytes(n, n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    t = C.Timer()
    for r in range(reps + 1):
        C.direct_step_dev(stream, n, tp.data_ptr(), tm.data_ptr(), 0, n, tv.data_ptr(), out.data_ptr(), None, 0.1, 0.001,
                          C.ARITH_AUTO, ws.data_ptr(), ws_bytes, t, uniform_mass=1.0)
        torch.cuda.synchronize()
        if r == 0:
            t.read()  # the first call (and its one-time costs) is not timed
    ms, cnt = t.read()
    for k in env:
        os.environ.pop(k, None)
    return ms / max(cnt, 1)


if __name__ == "__main__":
    sizes = [int(a) for a in sys.argv[1:]] or [65536, 131072, 196608, 262144, 327680, 393216, 524288]
    print(f"{'n':>9} {'stream ms':>10} {'mutual ms':>10} {'speed-up':>9}")
    for n in sizes:
        a = time_step(n, {"NBODY_DIRECT_ASM": 3})
        b = time_step(n, {"NBODY_DIRECT_ASM": 4, "NBODY_DIRECT_MUTUAL_MIN_N": 0})
        print(f"{n:>9} {a:10.3f} {b:10.3f} {a / b:9.3f}", flush=True)
