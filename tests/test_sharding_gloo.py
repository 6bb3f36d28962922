"""world_size-2 (and 3, 4, 8: the node the driver scales to) test of the target sharding + per-step position all-gather, on CPU with gloo.

The compute engine injected here is the CPU oracle (test infrastructure); what is under test is
nbody_simulation_amd/sharding.py: block partition, replicated sources, in-place velocity ownership and the
exchange.  The sharded run must equal the single-rank oracle trajectory bit for bit."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class OracleBackend:
    """CPU stand-in with HipBackend's prep/run signatures (EXACT arithmetic semantics)."""

    def prep(self, pos_all, mass_all, n):
        pass

    def run(self, pos_all, mass_all, n, begin, count, vel_block, out_block, dt):
        from oracle import oracle as orc
        pos = pos_all.numpy()[:n]
        w = mass_all.numpy()[:n].astype(np.uint32)
        acc, _ = orc.direct_accel(pos, w, targets=np.arange(begin, begin + count))
        acc = acc.astype(np.float32)
        d = np.float32(dt)
        v = vel_block.numpy() + acc * d
        p = pos[begin:begin + count] + v * d
        vel_block.copy_(torch.from_numpy(v))
        out_block.copy_(torch.from_numpy(p))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(fn, make_args, nprocs):
    """mp.spawn with a rendezvous port probed just before: between the probe and the children's bind another process can take the
    port (seen once on the GPU box: EADDRINUSE in the TCPStore, before any rank had touched the GPU).  That — and only that — is
    tried again with a fresh port; any other failure is the test's."""
    for attempt in range(3):
        try:
            mp.spawn(fn, args=make_args(_free_port()), nprocs=nprocs, join=True)
            return
        except Exception as e:  # noqa: BLE001
            if "EADDRINUSE" not in str(e) or attempt == 2:
                raise


def _worker(rank, world, port, n, steps, ret, chunks=0):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import nbody_simulation_amd as nb
    from nbody_simulation_amd.sharding import ShardedDirectStepper
    pos, vel, w = nb.scenes.plummer(n, seed=61)
    w = (np.arange(n) % 3 + 1).astype(np.uint32)
    st = ShardedDirectStepper(pos, vel, w, rank=rank, world=world, device=torch.device("cpu"),
                              backend=OracleBackend(), group=dist.group.WORLD, chunks=chunks)
    for _ in range(steps):
        st.step(0.1)
    p, v = st.local_state()
    ret[rank] = (p, v, st.all_positions(), st.local_rows())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n,chunks", [(2, 512, 0), (4, 512, 0), (2, 700, 3), (4, 333, 2), (3, 50, 1), (8, 1000, 2)])
def test_sharded_steps_equal_single_rank(world, n, chunks, orc, nb):
    """Block layout {c*G + r}, ragged sizes (short and empty blocks) and several chunks per step included."""
    steps = 3
    mgr = mp.Manager()
    ret = mgr.dict()
    _spawn(_worker, lambda port: (world, port, n, steps, ret, chunks), world)
    pos, vel, _ = nb.scenes.plummer(n, seed=61)
    w = (np.arange(n) % 3 + 1).astype(np.uint32)
    rp, rv, _ = orc.update_direct(pos, vel, w, delta=0.1, nsteps=steps)
    owned = np.zeros(n, int)
    for r in range(world):
        p, v, allp, rows = ret[r]
        owned[rows] += 1
        assert np.array_equal(p, rp[rows])
        assert np.array_equal(v, rv[rows])
        assert np.array_equal(allp, rp)          # every rank holds the same gathered positions
    assert np.all(owned == 1)                    # every body has exactly one owner


def _dump_worker(rank, world, port, n, steps, ret, chunks):
    """bench.py --dump-outputs on a sharded run: every rank joins the velocity collection, all ranks see the whole state."""
    import importlib.util
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    import nbody_simulation_amd as nb
    from nbody_simulation_amd.sharding import ShardedDirectStepper
    pos, vel, w = nb.scenes.plummer(n, seed=62)
    st = ShardedDirectStepper(pos, vel, w, rank=rank, world=world, device=torch.device("cpu"),
                              backend=OracleBackend(), group=dist.group.WORLD, chunks=chunks)
    for _ in range(steps):
        st.step(0.1)
    ret[rank] = bench._stepper_state(st, world)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n,chunks", [(1, 300, 0), (3, 333, 2)])
def test_bench_dump_state_is_the_whole_trajectory_in_input_order(world, n, chunks, orc, nb):
    steps = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    _spawn(_dump_worker, lambda port: (world, port, n, steps, ret, chunks), world)
    pos, vel, w = nb.scenes.plummer(n, seed=62)
    rp, rv, _ = orc.update_direct(pos, vel, w, delta=0.1, nsteps=steps)
    for r in range(world):
        p, v = ret[r]
        assert p.dtype == np.float32 and v.dtype == np.float32 and p.shape == v.shape == (n, 2)
        assert np.array_equal(p, rp) and np.array_equal(v, rv)


def test_block_layout(nb):
    from nbody_simulation_amd.sharding import block_layout
    assert block_layout(1 << 20, 1) == (1, 1 << 20)
    assert block_layout(1 << 20, 8) == (1, 131072)              # the headline config on 8 ranks: one chunk
    assert block_layout(1 << 24, 8) == (8, 262144)              # config 5: eight chunks of 262 144 targets per rank
    assert block_layout(1000, 4) == (1, 256)
    assert block_layout(0, 2) == (1, 64)
    for n, g, c in [(1, 1, 0), (63, 4, 4), (70001, 8, 2), (151405, 3, 0)]:
        cc, b = block_layout(n, g, c)
        assert b % 64 == 0 and g * cc * b >= n and (c == 0 or cc == c)


def test_hip_backend_refuses_cpu(nb):
    from nbody_simulation_amd.sharding import HipBackend
    with pytest.raises(nb._capi.NBodyError):
        HipBackend(torch.device("cpu"), 16, 16, 16, 0.001, 0)
