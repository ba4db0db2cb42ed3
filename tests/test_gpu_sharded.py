"""The sharded sweep on ONE GPU: several in-process ranks bound to the same statistics buffer
(the collective becomes shared memory), against the unsharded sweep; the RCCL all-gather path itself
with a 1-rank process group; three OS processes with the messages carried over gloo -- through the
torch.distributed driver and through the C library's own driver (icm_comm_init_transport)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _workload():
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip.synthetic import make_workload
    wl = make_workload(1900, 100, 180)  # lane, turn (some poses see nothing), lane
    return wl, ConfigICM(D=wl.config)


def _single(wl, cfg, sweeps):
    from icmslam_hip import SweepEngine
    eng = SweepEngine(cfg)
    eng.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
    eng.set_state(wl.map_init, wl.x_init, wl.x0)
    for _ in range(sweeps):
        eng.sweep_device("redblack")
    out = eng.get_state()
    eng.close()
    return out


@pytest.mark.parametrize("world", [2, 3, 4, 7])      # 7: shards of 272 poses and a last one of 268
def test_virtual_ranks_match_unsharded(world):
    import torch
    from icmslam_hip import SweepEngine
    from icmslam_hip.sharded import NoComm, ShardedSweep, partition, run_virtual_ranks
    wl, cfg = _workload()
    sweeps = 3
    x1, m1, c1, K1 = _single(wl, cfg, sweeps)
    blk, parts = partition(wl.T, world)
    assert blk % 2 == 0 and all(a % 2 == 0 for a, _ in parts), "shards are cut at even poses"
    engines, runners, stats = [], [], None
    for r, (a, b) in enumerate(parts):
        e = SweepEngine(cfg)
        e.upload(wl.scans[a:b], wl.odometry, wl.u, t_begin=a, t_end=b, pose_major=True, ghost_scan=wl.scans[a - 1] if a else None)
        run = ShardedSweep(e, r, world, wl.T, comm=NoComm(), stats=stats)
        stats = run.stats
        run.set_state(wl.map_init, wl.x_init, wl.x0)
        engines.append(e)
        runners.append(run)
    run_virtual_ranks(runners, sweeps)
    torch.cuda.synchronize()
    assert all(e.entry_path() == "hier" for e in engines), "the sharded sweep runs the hierarchical pipeline"
    for e in engines:
        x, m, c, K = e.get_state()
        assert K == K1
        assert np.abs(m[:, :K] - m1[:, :K1]).max() <= 1e-9
        assert np.array_equal(c, c1)
        d = np.abs(x - x1).max(axis=0)
        print("world %d: max|dx| %.3e, poses above 1e-9: %d" % (world, d.max(), int((d > 1e-9).sum())))
        assert d.max() <= 1e-9
    for e in engines:
        e.close()


@pytest.mark.parametrize("case", ["blind boundaries", "odd length", "five poses, one-pose last shard"])
def test_virtual_ranks_edge_shards(case):
    """Shard boundaries where it hurts: the ghost pose, the shard's first pose and its last pose WITHOUT kept beams (the
    reference's midpoint rule, scripts/ICM_ROS.py:143-147, on both sides of a cut); a sequence of odd length whose last
    shard is a single pose (solved one-sided from its ghost)."""
    import torch
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.sharded import NoComm, ShardedSweep, partition, run_virtual_ranks
    from icmslam_hip.synthetic import make_workload
    wl, cfg = _workload()
    scans, T = wl.scans.copy(), wl.T
    world = 3
    if case == "blind boundaries":
        _, parts = partition(T, world)
        for a, b in parts[1:]:
            scans[a - 2:a + 1] = 10.0            # poses a - 2, a - 1 (the ghost) and a see nothing
    elif case == "odd length":
        T = 1269                                 # blocks of 424: the last pose (1268, even) is solved one-sided
        scans = scans[:T]
        assert partition(T, world)[1][2] == (848, 1269)
    else:
        T = 5                                    # [0, 2) [2, 4) [4, 5): the last rank owns ONE pose, the sequence's last
        scans = scans[:T]
        assert partition(T, world)[1] == [(0, 2), (2, 4), (4, 5)]
    odo, u, x_init = wl.odometry[:, :T], wl.u[:, :T], np.ascontiguousarray(wl.x_init[:, :T])
    sweeps = 3
    e1 = SweepEngine(cfg)
    e1.upload(scans, odo, u, pose_major=True)
    e1.set_state(wl.map_init, x_init, wl.x0)
    for _ in range(sweeps):
        e1.sweep_device("redblack")
    x1, m1, c1, K1 = e1.get_state()
    e1.close()
    _, parts = partition(T, world)
    engines, runners, stats = [], [], None
    for r, (a, b) in enumerate(parts):
        e = SweepEngine(cfg)
        e.upload(scans[a:b], odo, u, t_begin=a, t_end=b, pose_major=True, ghost_scan=scans[a - 1] if a else None)
        run = ShardedSweep(e, r, world, T, comm=NoComm(), stats=stats)
        stats = run.stats
        run.set_state(wl.map_init, x_init, wl.x0)
        engines.append(e)
        runners.append(run)
    run_virtual_ranks(runners, sweeps)
    torch.cuda.synchronize()
    for e in engines:
        x, m, c, K = e.get_state()
        d = np.abs(x - x1).max(axis=0)
        print("%s: max|dx| %.3e, poses above 1e-9: %d" % (case, d.max(), int((d > 1e-9).sum())))
        assert K == K1 and np.array_equal(c, c1) and np.abs(m[:, :K] - m1[:, :K1]).max() <= 1e-9
        assert d.max() <= 1e-9
        e.close()


def test_rccl_all_gather_path_one_rank():
    """ShardedSweep with the real torch.distributed 'nccl' (= RCCL) backend, world size 1:
    same result as the plain device-resident sweep."""
    import torch
    import torch.distributed as dist
    from icmslam_hip import SweepEngine
    from icmslam_hip.sharded import ShardedSweep
    wl, cfg = _workload()
    x1, m1, c1, K1 = _single(wl, cfg, 2)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29517", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        e = SweepEngine(cfg)
        e.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
        run = ShardedSweep(e, 0, 1, wl.T)
        run.set_state(wl.map_init, wl.x_init, wl.x0)
        for _ in range(2):
            run.sweep("redblack")
        torch.cuda.synchronize()
        x, m, c, K = run.get_state()
        e.close()
    finally:
        dist.destroy_process_group()
    assert K == K1 and np.array_equal(x, x1) and np.array_equal(m, m1)


def test_library_collectives_one_rank():
    """The collectives issued by the C library itself (icm_comm_init / icm_sweep_sharded /
    icm_gather_poses: RCCL resolved with dlopen, all-gathers on the handle's stream), world size 1 --
    no torch.distributed anywhere: same state as the plain device-resident sweep, bit for bit."""
    from icmslam_hip import SweepEngine
    from icmslam_hip.sharded import LibrarySweep
    wl, cfg = _workload()
    x1, m1, c1, K1 = _single(wl, cfg, 3)
    e = SweepEngine(cfg)
    assert e.comm_available()
    e.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
    run = LibrarySweep(e, 0, 1, wl.T, bcast=lambda payload: payload)
    run.set_state(wl.map_init, wl.x_init, wl.x0)
    for _ in range(3):
        run.sweep("redblack")
    x, m, c, K = run.get_state()
    run.close()
    e.close()
    assert K == K1 and np.array_equal(x, x1) and np.array_equal(m, m1) and np.array_equal(c, c1)


def test_library_collectives_refuse_a_wrong_partition():
    from icmslam_hip import SweepEngine
    from icmslam_hip.engine import IcmError
    wl, cfg = _workload()
    e = SweepEngine(cfg)
    e.upload(wl.scans[:100], wl.odometry, wl.u, t_begin=0, t_end=100, pose_major=True)
    uid = e.comm_unique_id()
    with pytest.raises((IcmError, ValueError)):
        e.comm_init(uid, 0, 1)          # 100 poses are not block 0 of a 1-rank partition of T poses
    with pytest.raises((IcmError, ValueError)):
        e.sweep_sharded()               # no communicator
    e.close()


def _native_worker(rank, world, port, out_path, driver):
    """One rank of a multi-process sharded sweep; every rank uses cuda:0 (one-GPU box), the messages travel over
    gloo through host memory.  driver "torch": ShardedSweep, the library writes its message into the send buffer
    (icm_bind_exchange_send) and the test's TorchComm gathers it; driver "library": icm_sweep_sharded -- ONE C call
    per sweep -- with the same gloo hop plugged in as the library's transport (icm_comm_init_transport)."""
    import ctypes
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "icm-slam_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    from icmslam_hip import SweepEngine
    from icmslam_hip.sharded import LibrarySweep, ShardedSweep, TorchComm, partition
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)

    class HostHopComm(TorchComm):
        """TorchComm whose all-gathers hop through host memory (gloo has no device collectives)."""

        def _ag(self, out, inp):
            o, i = out.cpu(), inp.cpu()
            self.dist.all_gather_into_tensor(o, i, group=self.group)
            out.copy_(o)

        def gather_stats(self, sw):
            assert sw.native
            self._ag(sw.stats, sw.stats_send)

        def all_gather(self, buf, r, count):
            mine = buf[r * count:(r + 1) * count].clone()
            self._ag(buf, mine)

    from util import hip_runtime
    hip = None   # (resolved at the first call: the runtime is loaded with the library)
    calls = []

    def gloo_transport(send_ptr, recv_ptr, count, stream_ptr):
        """icm_allgather_fn: wait for the handle's stream, device -> host, gloo all-gather, host -> device."""
        hip = hip_runtime()
        assert hip.hipStreamSynchronize(ctypes.c_void_p(stream_ptr)) == 0
        mine = torch.empty(count, dtype=torch.float64)
        allr = torch.empty(count * world, dtype=torch.float64)
        assert hip.hipMemcpy(ctypes.c_void_p(mine.data_ptr()), ctypes.c_void_p(send_ptr), ctypes.c_size_t(8 * count), 2) == 0   # D2H
        dist.all_gather_into_tensor(allr, mine)
        assert hip.hipMemcpy(ctypes.c_void_p(recv_ptr), ctypes.c_void_p(allr.data_ptr()), ctypes.c_size_t(8 * count * world), 1) == 0   # H2D
        calls.append(count)

    wl, cfg = _workload()
    _, parts = partition(wl.T, world)
    a, b = parts[rank]
    e = SweepEngine(cfg)
    e.upload(wl.scans[a:b], wl.odometry, wl.u, t_begin=a, t_end=b, pose_major=True, ghost_scan=wl.scans[a - 1] if a else None)
    if driver == "library":
        run = LibrarySweep(e, rank, world, wl.T, transport=gloo_transport)
    else:
        run = ShardedSweep(e, rank, world, wl.T, comm=HostHopComm())
        assert run.native
    run.set_state(wl.map_init, wl.x_init, wl.x0)
    sweeps = 3
    for _ in range(sweeps):
        run.sweep("redblack")
    torch.cuda.synchronize()
    if driver == "library":
        assert calls == [e.stats_stride()] * sweeps, "exactly one collective per sweep: %r" % (calls,)
    x, m, c, K = run.get_state()
    np.savez(out_path % rank, x=x, m=m[:, :K], c=c, K=K, path=e.entry_path())
    # the per-rank phase report bench.py prints at N > 1 (icm_set_phase_timing): two more sweeps with events at the phase boundaries
    e.set_phase_timing(True)
    for _ in range(2):
        run.sweep("redblack")
    ph, n = e.phase_times()
    e.set_phase_timing(False)
    print("rank %d phases (ms per sweep): %s" % (rank, ph))
    assert n == 2 and all(v >= 0.0 for v in ph.values()) and ph["local"] > 0.0 and ph["solve"] > 0.0
    e.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("driver", ["torch", "library"])
def test_three_processes_one_collective_per_sweep(tmp_path, driver):
    """Three OS processes (ranks) on the one GPU, real exchanges between them (gloo): one all-gather per sweep, the
    shard's ghost pose instead of a halo exchange -- the unsharded result; the interior rank has a neighbour on both
    sides.  "library": the C library's sharded driver (icm_sweep_sharded) at world size 3, its collective carried by
    the transport hook."""
    import torch.multiprocessing as mp
    world = 3
    wl, cfg = _workload()
    x1, m1, c1, K1 = _single(wl, cfg, 3)
    out = str(tmp_path / "rank%d.npz")
    mp.spawn(_native_worker, args=(world, 29561 if driver == "torch" else 29571, out, driver), nprocs=world, join=True)
    res = [np.load(out % r) for r in range(world)]
    for r, g in enumerate(res):
        assert str(g["path"]) == "hier"
        assert int(g["K"]) == K1 and np.array_equal(g["c"], c1)
        assert np.abs(g["m"] - m1[:, :K1]).max() <= 1e-9
        d = np.abs(g["x"] - x1).max(axis=0)
        print("%s rank %d: max|dx| %.3e, poses above 1e-9: %d" % (driver, r, d.max(), int((d > 1e-9).sum())))
        assert d.max() <= 1e-9
    for g in res[1:]:
        assert np.array_equal(g["x"], res[0]["x"]) and np.array_equal(g["m"], res[0]["m"])   # replicas agree bit for bit


def _failing_worker(rank, world, port, out_path):
    """Careful-form failure on ONE rank (its labels exceed L): every rank must come back with the error instead of
    waiting in the collective."""
    import ctypes
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "icm-slam_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.sharded import LibrarySweep, partition
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    from util import hip_runtime
    hip = None   # (resolved at the first call: the runtime is loaded with the library)

    def gloo_transport(send_ptr, recv_ptr, count, stream_ptr):
        hip = hip_runtime()
        assert hip.hipStreamSynchronize(ctypes.c_void_p(stream_ptr)) == 0
        mine = torch.empty(count, dtype=torch.float64)
        allr = torch.empty(count * world, dtype=torch.float64)
        assert hip.hipMemcpy(ctypes.c_void_p(mine.data_ptr()), ctypes.c_void_p(send_ptr), ctypes.c_size_t(8 * count), 2) == 0
        dist.all_gather_into_tensor(allr, mine)
        assert hip.hipMemcpy(ctypes.c_void_p(recv_ptr), ctypes.c_void_p(allr.data_ptr()), ctypes.c_size_t(8 * count * world), 1) == 0

    wl, _ = _workload()
    conf = dict(wl.config)
    conf["L"] = wl.K + 2          # room for two new landmarks only
    cfg = ConfigICM(D=conf)
    _, parts = partition(wl.T, world)
    a, b = parts[rank]
    e = SweepEngine(cfg)
    e.upload(wl.scans[a:b], wl.odometry, wl.u, t_begin=a, t_end=b, pose_major=True, ghost_scan=wl.scans[a - 1] if a else None)
    run = LibrarySweep(e, rank, world, wl.T, transport=gloo_transport)
    x = wl.x_init.copy()
    # poses of rank 1's block pushed 3 m sideways: every one of its scans leaves the gate and creates a landmark
    a1, b1 = parts[1]
    x[1, a1:b1] += 3.0
    run.set_state(wl.map_init, x, wl.x0)
    outcome = "ok"
    try:
        run.sweep("redblack")
    except IndexError as ex:
        outcome = "IndexError: " + str(ex)
    open(out_path % rank, "w").write(outcome)
    e.close()
    dist.barrier()
    dist.destroy_process_group()


def test_a_rank_local_failure_is_collective(tmp_path):
    """One rank's labels exceed L in phase A (the reference's IndexError, scripts/ICM_SLAM_tools.py:191): it still takes
    part in the sweep's collective with the error code in its header, and every rank raises -- nobody hangs."""
    import torch.multiprocessing as mp
    world = 3
    out = str(tmp_path / "rank%d.txt")
    mp.spawn(_failing_worker, args=(world, 29581, out), nprocs=world, join=True)
    res = [open(out % r).read() for r in range(world)]
    print(res)
    assert all(r.startswith("IndexError") for r in res), res


def _protocol_worker(rank, world, port, out_path, driver, case):
    """One rank of a three-process job in which ONE rank cannot finish phase A of the sweep's FIRST attempt (the one
    every rank queues whole): case "hip" -- rank 1's device reports an error (icm_set_fault); case "nobeam" -- the
    sequence's last pose has no kept beams (the reference's IndexError, scripts/ICM_ROS.py:144: a property of the data
    that only the owner of the last block sees).  Every rank must come back with the error; nobody may wait in a second
    collective for a rank that has left."""
    import ctypes
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "icm-slam_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    from icmslam_hip import SweepEngine
    from icmslam_hip.sharded import LibrarySweep, ShardedSweep, TorchComm, partition
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    from util import hip_runtime

    class HostHopComm(TorchComm):
        def _ag(self, out, inp):
            o, i = out.cpu(), inp.cpu()
            self.dist.all_gather_into_tensor(o, i, group=self.group)
            out.copy_(o)

        def gather_stats(self, sw):
            self._ag(sw.stats, sw.stats_send)

        def all_gather(self, buf, r, count):
            self._ag(buf, buf[r * count:(r + 1) * count].clone())

    calls = []

    def gloo_transport(send_ptr, recv_ptr, count, stream_ptr):
        hip = hip_runtime()
        assert hip.hipStreamSynchronize(ctypes.c_void_p(stream_ptr)) == 0
        mine = torch.empty(count, dtype=torch.float64)
        allr = torch.empty(count * world, dtype=torch.float64)
        assert hip.hipMemcpy(ctypes.c_void_p(mine.data_ptr()), ctypes.c_void_p(send_ptr), ctypes.c_size_t(8 * count), 2) == 0
        dist.all_gather_into_tensor(allr, mine)
        assert hip.hipMemcpy(ctypes.c_void_p(recv_ptr), ctypes.c_void_p(allr.data_ptr()), ctypes.c_size_t(8 * count * world), 1) == 0
        calls.append(count)

    wl, cfg = _workload()
    scans = wl.scans
    _, parts = partition(wl.T, world)
    a, b = parts[rank]
    e = SweepEngine(cfg)
    e.upload(scans[a:b], wl.odometry, wl.u, t_begin=a, t_end=b, pose_major=True, ghost_scan=scans[a - 1] if a else None)
    run = LibrarySweep(e, rank, world, wl.T, transport=gloo_transport) if driver == "library" else ShardedSweep(e, rank, world, wl.T, comm=HostHopComm())
    run.set_state(wl.map_init, wl.x_init, wl.x0)
    run.sweep("redblack")             # a clean sweep first: the job is in its steady state (sweeps queued whole)
    if case == "hip" and rank == 1:
        e.set_fault(1)
    outcome = "ok"
    try:
        run.sweep("redblack")
    except (IndexError, RuntimeError) as ex:
        outcome = "%s: %s" % (type(ex).__name__, ex)
    open(out_path % rank, "w").write(outcome + "\ncollectives=%d" % len(calls))
    e.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("driver,case,port", [("library", "hip", 29601), ("torch", "hip", 29611), ("library", "nobeam", 29621), ("torch", "nobeam", 29631)])
def test_a_rank_that_fails_in_a_sweep_queued_whole_takes_every_rank_with_it(tmp_path, driver, case, port):
    """The first attempt of a sharded sweep is queued whole on every rank.  A rank that fails in it on its own -- a
    device error, or the no-beam last pose only the last block's owner sees -- sends its message with the error code
    and leaves; its peers, to whom the code reads as "flags set: repeat the sweep", must find the code in the headers
    BEFORE they start the repeated sweep's collective, and leave with the same error (round 3 hung here)."""
    import torch.multiprocessing as mp
    world = 3
    out = str(tmp_path / "rank%d.txt")
    mp.spawn(_protocol_worker_entry, args=(world, port, out, driver, case), nprocs=world, join=True)
    res = [open(out % r).read() for r in range(world)]
    print(driver, case, res)
    want = "IcmError: icmslam_hip error -2" if case == "hip" else "IndexError"      # (IcmError is a RuntimeError)
    assert all(r.startswith(want) for r in res), res


def _protocol_worker_entry(rank, world, port, out_path, driver, case):
    if case == "nobeam":
        _nobeam_worker(rank, world, port, out_path, driver)
    else:
        _protocol_worker(rank, world, port, out_path, driver, case)


def _post_exchange_worker(rank, world, port, out_path, driver, then):
    """One rank of a three-process job in which rank 1 fails BEHIND a sweep's exchange (icm_set_fault(2): its
    icm_sweep_targets reports a device error while its peers' phases run to the end).  `then` = what the peers do next:
    "sweep" -- another sweep; "end" -- the closing exchange (get_state).  Rank 1 must come back with its error, and the
    peers with the same error at their next exchange; nobody may hang."""
    import ctypes
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "icm-slam_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    from icmslam_hip import SweepEngine
    from icmslam_hip.sharded import LibrarySweep, ShardedSweep, TorchComm, partition
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    from util import hip_runtime

    class HostHopComm(TorchComm):
        def _ag(self, out, inp):
            o, i = out.cpu(), inp.cpu()
            self.dist.all_gather_into_tensor(o, i, group=self.group)
            out.copy_(o)

        def gather_stats(self, sw):
            self._ag(sw.stats, sw.stats_send)

        def all_gather(self, buf, r, count):
            self._ag(buf, buf[r * count:(r + 1) * count].clone())

    def gloo_transport(send_ptr, recv_ptr, count, stream_ptr):
        hip = hip_runtime()
        assert hip.hipStreamSynchronize(ctypes.c_void_p(stream_ptr)) == 0
        mine = torch.empty(count, dtype=torch.float64)
        allr = torch.empty(count * world, dtype=torch.float64)
        assert hip.hipMemcpy(ctypes.c_void_p(mine.data_ptr()), ctypes.c_void_p(send_ptr), ctypes.c_size_t(8 * count), 2) == 0
        dist.all_gather_into_tensor(allr, mine)
        assert hip.hipMemcpy(ctypes.c_void_p(recv_ptr), ctypes.c_void_p(allr.data_ptr()), ctypes.c_size_t(8 * count * world), 1) == 0

    wl, cfg = _workload()
    _, parts = partition(wl.T, world)
    a, b = parts[rank]
    e = SweepEngine(cfg)
    e.upload(wl.scans[a:b], wl.odometry, wl.u, t_begin=a, t_end=b, pose_major=True, ghost_scan=wl.scans[a - 1] if a else None)
    run = LibrarySweep(e, rank, world, wl.T, transport=gloo_transport) if driver == "library" else ShardedSweep(e, rank, world, wl.T, comm=HostHopComm())
    run.set_state(wl.map_init, wl.x_init, wl.x0)
    run.sweep("redblack")             # a clean sweep first
    if rank == 1:
        e.set_fault(2)
    log = []
    try:
        run.sweep("redblack")         # rank 1 fails behind this sweep's exchange; its peers finish the sweep
        log.append("sweep ok")
        if then == "sweep":
            run.sweep("redblack")     # the peers' next exchange: rank 1's farewell
            log.append("next sweep ok")
        else:
            run.get_state()           # ... or the closing exchange
            log.append("end ok")
    except (IndexError, RuntimeError) as ex:
        log.append("%s: %s" % (type(ex).__name__, ex))
    open(out_path % rank, "w").write(" | ".join(log))
    e.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("driver,then,port", [("library", "sweep", 29641), ("torch", "sweep", 29651), ("library", "end", 29661), ("torch", "end", 29671)])
def test_a_rank_that_fails_behind_the_exchange_takes_every_rank_with_it(tmp_path, driver, then, port):
    """A device error in one rank's icm_sweep_targets -- behind the sweep's one collective, where its peers no longer
    depend on it in this sweep (scripts/ICM_ROS.py:141-158 sharded) -- must still end every rank: the failing rank sends a
    farewell message into the peers' NEXT exchange (the next sweep's, or the closing one) and every rank raises its error
    there.  Round 4 left the peers waiting in the next sweep's all-gather."""
    import torch.multiprocessing as mp
    world = 3
    out = str(tmp_path / "rank%d.txt")
    mp.spawn(_post_exchange_worker, args=(world, port, out, driver, then), nprocs=world, join=True)
    res = [open(out % r).read() for r in range(world)]
    print(driver, then, res)
    assert res[1].startswith("IcmError: icmslam_hip error -2"), res          # the failing rank: its own error, at once
    for r in (0, 2):
        assert res[r].startswith("sweep ok | IcmError: icmslam_hip error -2"), res   # the peers: one exchange later


def _nobeam_worker(rank, world, port, out_path, driver):
    """case "nobeam" of _protocol_worker without the clean sweep in front (the last pose never has beams)."""
    import ctypes
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "icm-slam_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    from icmslam_hip import SweepEngine
    from icmslam_hip.sharded import LibrarySweep, ShardedSweep, TorchComm, partition
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    from util import hip_runtime

    class HostHopComm(TorchComm):
        def _ag(self, out, inp):
            o, i = out.cpu(), inp.cpu()
            self.dist.all_gather_into_tensor(o, i, group=self.group)
            out.copy_(o)

        def gather_stats(self, sw):
            self._ag(sw.stats, sw.stats_send)

        def all_gather(self, buf, r, count):
            self._ag(buf, buf[r * count:(r + 1) * count].clone())

    def gloo_transport(send_ptr, recv_ptr, count, stream_ptr):
        hip = hip_runtime()
        assert hip.hipStreamSynchronize(ctypes.c_void_p(stream_ptr)) == 0
        mine = torch.empty(count, dtype=torch.float64)
        allr = torch.empty(count * world, dtype=torch.float64)
        assert hip.hipMemcpy(ctypes.c_void_p(mine.data_ptr()), ctypes.c_void_p(send_ptr), ctypes.c_size_t(8 * count), 2) == 0
        dist.all_gather_into_tensor(allr, mine)
        assert hip.hipMemcpy(ctypes.c_void_p(recv_ptr), ctypes.c_void_p(allr.data_ptr()), ctypes.c_size_t(8 * count * world), 1) == 0

    wl, cfg = _workload()
    scans = wl.scans.copy()
    scans[-1, :] = 1e3                # beyond rango_laser_max: filtrar_z keeps nothing of the last scan
    _, parts = partition(wl.T, world)
    a, b = parts[rank]
    e = SweepEngine(cfg)
    e.upload(scans[a:b], wl.odometry, wl.u, t_begin=a, t_end=b, pose_major=True, ghost_scan=scans[a - 1] if a else None)
    run = LibrarySweep(e, rank, world, wl.T, transport=gloo_transport) if driver == "library" else ShardedSweep(e, rank, world, wl.T, comm=HostHopComm())
    run.set_state(wl.map_init, wl.x_init, wl.x0)
    outcome = "ok"
    try:
        run.sweep("redblack")
    except (IndexError, RuntimeError) as ex:
        outcome = "%s: %s" % (type(ex).__name__, ex)
    open(out_path % rank, "w").write(outcome)
    e.close()
    dist.barrier()
    dist.destroy_process_group()


def _s2_worker(rank, world, port, out_path):
    """One of `world` OS processes, each holding one block of the full S2 sequence on cuda:0: icm_sweep_sharded (sweeps
    queued whole) with its collective carried over gloo."""
    import ctypes
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "icm-slam_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.sharded import LibrarySweep, partition
    from icmslam_hip.synthetic import WORKLOADS, make_workload
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    from util import hip_runtime
    calls = []

    def gloo_transport(send_ptr, recv_ptr, count, stream_ptr):
        hip = hip_runtime()
        assert hip.hipStreamSynchronize(ctypes.c_void_p(stream_ptr)) == 0
        mine = torch.empty(count, dtype=torch.float64)
        allr = torch.empty(count * world, dtype=torch.float64)
        assert hip.hipMemcpy(ctypes.c_void_p(mine.data_ptr()), ctypes.c_void_p(send_ptr), ctypes.c_size_t(8 * count), 2) == 0
        dist.all_gather_into_tensor(allr, mine)
        assert hip.hipMemcpy(ctypes.c_void_p(recv_ptr), ctypes.c_void_p(allr.data_ptr()), ctypes.c_size_t(8 * count * world), 1) == 0
        calls.append(count)

    wl = make_workload(*WORKLOADS["S2"])
    cfg = ConfigICM(D=wl.config)
    _, parts = partition(wl.T, world)
    a, b = parts[rank]
    e = SweepEngine(cfg)
    e.upload(wl.scans[a:b], wl.odometry, wl.u, t_begin=a, t_end=b, pose_major=True, ghost_scan=wl.scans[a - 1] if a else None)
    del wl.scans
    run = LibrarySweep(e, rank, world, wl.T, transport=gloo_transport)
    run.set_state(wl.map_init, wl.x_init, wl.x0)
    states = []
    for _ in range(2):
        run.sweep("redblack")
        # (the pose blocks travel with get_state: a collective of its own, outside the sweep)
        n0 = len(calls)
        states.append(run.get_state())
        del calls[n0:]
    assert calls == [e.stats_stride()] * 2, "one collective per sweep: %r" % (calls,)
    (x1, m1, c1, K1), (x2, m2, c2, K2) = states
    np.savez(out_path % rank, x1=x1, m1=m1[:, :K1], c1=c1, K1=K1, x2=x2, m2=m2[:, :K2], c2=c2, K2=K2, path=e.entry_path(), deferred=e.fused_deferred())
    e.close()
    dist.barrier()
    dist.destroy_process_group()


def test_full_s2_in_four_processes_through_the_library_driver(tmp_path):
    """BASELINE configs[4]'s job -- the full 100 000-pose sequence, pose-sharded -- as FOUR OS processes on the one GPU
    (the box allows six), each driving icm_sweep_sharded on its 25 000-pose block with every sweep queued whole and the
    collective carried between the processes over gloo: poses, map and counters after sweeps 1 and 2 against the C
    oracle's full-size fixture, replicas bit-equal."""
    import torch.multiprocessing as mp
    from util import GOLD
    world = 4
    out = str(tmp_path / "s2rank%d.npz")
    mp.spawn(_s2_worker, args=(world, 29651, out), nprocs=world, join=True)
    fx = np.load(os.path.join(GOLD, "s2_fullsize.npz"))
    res = [np.load(out % r) for r in range(world)]
    for r, g in enumerate(res):
        assert str(g["path"]) == "hier"
        for s in ("1", "2"):
            K = int(g["K" + s])
            d = np.abs(g["x" + s] - fx["x" + s]).max(axis=0)
            if r == 0:
                print("S2 in %d processes vs C oracle after sweep %s: K %d/%d  max|dmap| %.2e  max|dx| %.3e  poses above 1e-9: %d"
                      % (world, s, K, int(fx["K" + s]), np.abs(g["m" + s] - fx["map" + s]).max(), d.max(), int((d > 1e-9).sum())))
            assert K == int(fx["K" + s]) and np.abs(g["m" + s] - fx["map" + s]).max() <= 1e-9 and d.max() <= 1e-9
            cs = g["c" + s]
            assert np.array_equal(cs[:fx["counts" + s].size], fx["counts" + s]) and not cs[fx["counts" + s].size:].any()
    for g in res[1:]:
        assert np.array_equal(g["x2"], res[0]["x2"]) and np.array_equal(g["m2"], res[0]["m2"])


@pytest.mark.parametrize("form", ["runs", "beams"])
def test_a_ghost_pose_is_solved_to_its_owners_value(form):
    """A shard solves the pose in front of it too (its ghost pose) instead of receiving it between the colours: same
    beams, same neighbours' values, the same additions over its entries as its owner -- and targets that are the same
    running means up to the rounding of differently associated sums.  Directly: after one sweep, before any rank's
    block reaches the others, rank r's own copy of pose a_r - 1 against rank r - 1's."""
    import torch
    from icmslam_hip import SweepEngine
    from icmslam_hip.sharded import NoComm, ShardedSweep, partition
    wl, cfg = _workload()
    world = 4
    _, parts = partition(wl.T, world)
    engines, runs, stats = [], [], None
    for r, (a, b) in enumerate(parts):
        e = SweepEngine(cfg)
        e.upload(wl.scans[a:b], wl.odometry, wl.u, t_begin=a, t_end=b, pose_major=True, ghost_scan=wl.scans[a - 1] if a else None)
        e.set_assoc_form(form)
        run = ShardedSweep(e, r, world, wl.T, comm=NoComm(), stats=stats)
        stats = run.stats
        run.set_state(wl.map_init, wl.x_init, wl.x0)
        engines.append(e)
        runs.append(run)
    for sweep in range(2):
        for e in engines:
            e.sweep_local()
        torch.cuda.synchronize()
        for e in engines:
            e.sweep_targets()
        for e in engines:
            e.sweep_solve("redblack", -1)
        for e in engines:
            e.sweep_finish()
        torch.cuda.synchronize()
        worst, equal = 0.0, 0
        for r in range(1, world):
            a = parts[r][0]
            ghost = runs[r].poses.view(-1, 3)[a - 1].cpu().numpy()
            owner = runs[r - 1].poses.view(-1, 3)[a - 1].cpu().numpy()
            worst = max(worst, float(np.abs(ghost - owner).max()))
            equal += int(np.array_equal(ghost, owner))
            assert not np.array_equal(owner, wl.x_init[:, a - 1]), "the pose was solved"
        print("sweep %d: ghost poses bit-equal to their owners' %d of %d, max |difference| %.2e" % (sweep + 1, equal, world - 1, worst))
        assert worst <= 1e-9
        n = runs[0].blk * 3          # the pose blocks reach the other ranks (get_state's all-gather)
        for src in runs:
            for dst in runs:
                if dst is not src:
                    dst.poses[src.rank * n:(src.rank + 1) * n].copy_(src.poses[src.rank * n:(src.rank + 1) * n])
        torch.cuda.synchronize()
    for e in engines:
        e.close()
