#!/usr/bin/env python3
"""Throughput of many independent sequences on one GPU (icm_init_pass_batch / icm_sweep_batch) against M single calls and
against the compiled C oracle on one host core.

    python tools/batch_timing.py [--sizes 1,4,16,64,256,1024] [--out profiles/batch_scaling.json]

M copies of data_IJAC2018, each at its own dist_thr (spread over [0.8, 1.2]), config_default.yaml otherwise.  Per M, in a
child process of its own under `timeout -k 10`: wall ms of one init_pass_batch and of one sweep_batch (the state restored
in front of each timed sweep), the sweep split into the chain launch(es) -- HIP events around them (icm_enable_timing on
the launch's first member, a run of its own) -- and the rest (every member's own phases, host included); device memory
per member; sequences per second; the ratio to M single calls (icm_init_pass, icm_sweep_device) and to the C oracle on
one core (bench.py's dataset_cpu_baseline_c, the figure bench.py records).  A size whose engines cannot be created or run
out of memory is recorded and ends the run: no retry, no larger size.  One JSON line goes to --out.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "icm-slam_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _hip():
    """The HIP runtime this process has loaded already (the copy libicmslam_hip.so is bound to)."""
    import ctypes
    for ln in open("/proc/self/maps"):
        path = ln.split()[-1]
        if "libamdhip64.so" in path and os.path.exists(path):
            return ctypes.CDLL(path)
    raise RuntimeError("no HIP runtime loaded")


def _free_bytes(hip):
    import ctypes
    f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
    if hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) != 0:
        return None
    return f.value


def one_size(M):
    """Runs in the child: the record of one batch size."""
    import numpy as np
    from ICM_SLAM_tools import ConfigICM, Mapa
    from icmslam_hip import SweepEngine, init_pass_batch, sweep_batch
    from util import dataset
    zz, odo, u = dataset()
    x0 = odo[:, 0]
    thrs = np.linspace(0.8, 1.2, M) if M > 1 else np.array([1.0])
    engines = []
    hip = None
    free0 = None
    rec = {"M": M}
    try:
        for t in thrs:
            cfg = ConfigICM("config_default.yaml")
            cfg.dist_thr = float(t)
            e = SweepEngine(cfg)
            if hip is None:
                hip = _hip()
                hip.hipDeviceSynchronize()
                free0 = _free_bytes(hip)
            engines.append(e)
            e.upload(zz, odo, u)
    except Exception as ex:   # noqa: BLE001  (recorded; the parent stops here)
        return {"M": M, "error": "engine creation: %s: %s" % (type(ex).__name__, ex), "created": len(engines)}
    sync = hip.hipDeviceSynchronize
    res = init_pass_batch(engines, [x0] * M)   # (warm-up, and the states the sweeps start from)
    bad = [r for r in res if isinstance(r, Exception)]
    if bad:
        return {"M": M, "error": "init pass: %s" % bad[0]}
    t0 = time.perf_counter()
    init_pass_batch(engines, [x0] * M)
    t_init = time.perf_counter() - t0
    for e, r in zip(engines, res):
        x, y, cnt, lact, _ = r
        mo = Mapa(e.config)
        mo.landmarks_actuales = lact
        mo.cant_obs_i = cnt
        yy = mo.filtrar(y)[:, :mo.landmarks_actuales]
        e.set_state(yy, x, x0, mo.landmarks_actuales)
        e.snapshot_state()
    sync()
    free1 = _free_bytes(hip)

    def timed_sweep():
        for e in engines:
            e.restore_state()
        sync()
        t0 = time.perf_counter()
        out = sweep_batch(engines)
        sync()
        el = time.perf_counter() - t0
        if any(r is not None for r in out):
            raise RuntimeError("sweep_batch: %s" % next(r for r in out if r is not None))
        return el

    timed_sweep()   # warm-up
    walls = sorted(timed_sweep() for _ in range(3))
    t_sweep = walls[1]
    # the chain launch(es) alone: events around them, booked on the members with timing on (one is enough)
    for e in engines:
        e.restore_state()
    sync()
    engines[0].enable_timing(True)   # (also resets the counters)
    sweep_batch(engines)
    sync()
    chain_ms = engines[0].kernel_times().get("k_solve", (float("nan"), 0))[0]
    engines[0].enable_timing(False)
    # one member's single calls
    e = engines[0]
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        e.init_pass(x0)
        sync()
        ts.append(time.perf_counter() - t0)
    single_init = sorted(ts)[1]
    ts = []
    for _ in range(3):
        e.restore_state()
        sync()
        t0 = time.perf_counter()
        e.sweep_device("sequential")
        sync()
        ts.append(time.perf_counter() - t0)
    single_sweep = sorted(ts)[1]
    rec.update({
        "init_pass_batch_ms": round(1e3 * t_init, 3),
        "sweep_batch_ms": round(1e3 * t_sweep, 3),
        "sweep_chain_launch_ms": round(chain_ms, 3),
        "sweep_member_phases_ms": round(1e3 * t_sweep - chain_ms, 3),
        "sweep_member_phases_ms_per_member": round((1e3 * t_sweep - chain_ms) / M, 4),
        "device_bytes_per_member": int((free0 - free1) / M) if free0 is not None and free1 is not None else None,
        "init_pass_seq_per_s": round(M / t_init, 2),
        "sweep_seq_per_s": round(M / t_sweep, 2),
        "single_init_pass_ms": round(1e3 * single_init, 3),
        "single_sweep_sequential_ms": round(1e3 * single_sweep, 3),
        "init_pass_over_M_single_calls": round(M * single_init / t_init, 2),
        "sweep_over_M_single_calls": round(M * single_sweep / t_sweep, 2),
    })
    for e in engines:
        e.close()
    return rec


def c_oracle_baseline():
    """bench.py's dataset_cpu_baseline_c on this host: ms of the init pass and of one sequential sweep, one core."""
    import numpy as np
    import bench
    from ICM_ROS import ICM_ROS
    from ICM_SLAM_tools import ConfigICM
    gold = os.path.join(ROOT, "tests", "golden")
    icm = ICM_ROS(ConfigICM("config_default.yaml"))
    icm.load_data(os.path.join(gold, "data_IJAC2018.npz"))
    init = np.load(os.path.join(gold, "init_pass.npz"))
    return bench.dataset_cpu_baseline_c(icm, init)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,4,16,64,256,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_scaling.json"))
    ap.add_argument("--timeout", type=int, default=600, help="seconds per size")
    ap.add_argument("--one", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        print("RESULT " + json.dumps(one_size(a.one)), flush=True)
        return
    sizes = [int(s) for s in a.sizes.split(",")]
    recs = []
    for M in sizes:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--one", str(M)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if p.returncode != 0 or line is None:
            tail = (p.stderr or p.stdout).strip().splitlines()[-3:]
            recs.append({"M": M, "error": "exit %d: %s" % (p.returncode, " | ".join(tail))})
            print(json.dumps(recs[-1]), flush=True)
            break
        r = json.loads(line[len("RESULT "):])
        recs.append(r)
        print(json.dumps(r), flush=True)
        if "error" in r:
            break
    cb = c_oracle_baseline()
    c_init, c_seq = cb["init_pass"]["ms"], cb["sequential"]["ms"]
    for r in recs:
        if "error" in r:
            continue
        r["init_pass_over_c_oracle_one_core"] = round(r["M"] * c_init / r["init_pass_batch_ms"], 2)
        r["sweep_over_c_oracle_one_core"] = round(r["M"] * c_seq / r["sweep_batch_ms"], 2)
    out = {"tool": "tools/batch_timing.py", "workload": "data_IJAC2018 x M, dist_thr spread over [0.8, 1.2]",
           "cpu_baseline_c": {"init_pass_ms": c_init, "sequential_ms": c_seq, "cores": 1, "host_cores": cb.get("host_cores")},
           "target": "M = 64: aggregate throughput >= 10x the C oracle on one core, init pass and sweep",
           "sizes": recs}
    try:
        from icmslam_hip import _lib
        out["build"] = _lib.load().icm_build_id().decode()
    except Exception:   # noqa: BLE001
        pass
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
