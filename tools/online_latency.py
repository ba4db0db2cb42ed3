"""Latency of the online initialisation (icm_online_*), on data_IJAC2018 and on a synthetic stream (B = 360).

Per stream:
  step_ms        wall time of one online_step (push + advance, both end in a host synchronisation) at 1, 8 and 64
                 samples per step: median and p99 over the steps after the first 5 (warm-up)
  advance_us     k_init_advance kernel time per sample (icm_enable_timing: HIP events around the launch), 8 per step
  whole_ms       one push + one advance of the whole sequence against icm_upload + icm_prefilter + icm_init_pass
  finish_ms      online_finish against icm_upload + icm_prefilter of the same arrays

    python tools/online_latency.py [--samples 20000] [--out profiles/online_latency.json]

Prints (and with --out writes) one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "icm-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from ICM_SLAM_tools import ConfigICM  # noqa: E402
from icmslam_hip import SweepEngine  # noqa: E402
from icmslam_hip.synthetic import make_workload  # noqa: E402


def _now():
    return time.perf_counter() * 1e3


def _stats(v):
    v = np.asarray(v)
    return {"median": round(float(np.median(v)), 4), "p99": round(float(np.percentile(v, 99)), 4), "n": int(v.size)}


def _stream(cfg, zz, odo, u):
    T = zz.shape[1]
    out = {"T": T, "B": zz.shape[0]}
    eng = SweepEngine(cfg)
    # per-step wall time
    steps = {}
    for k in (1, 8, 64):
        eng.online_begin(zz.shape[0], capacity=1024)
        t, times = 0, []
        while t + k <= T and len(times) < 2000:
            a = _now()
            eng.online_push(zz[:, t:t + k], odo[:, t:t + k], u[:, t:t + k])
            eng.online_advance()
            times.append(_now() - a)
            t += k
        steps[str(k)] = _stats(times[5:])
    out["step_ms"] = steps
    # kernel time per sample
    eng.online_begin(zz.shape[0], capacity=1024)
    eng.online_push(zz[:, :1], odo[:, :1], u[:, :1])
    eng.enable_timing(True)
    n = min(T, 4001)
    for t in range(1, n, 8):
        e = min(t + 8, n)
        eng.online_push(zz[:, t:e], odo[:, t:e], u[:, t:e])
        eng.online_advance()
    ms, launches = eng.kernel_times()["k_init_advance"]
    eng.enable_timing(False)
    out["advance_us_per_sample"] = round(1e3 * ms / (n - 1), 3)
    out["advance_launches"] = int(launches)
    # the whole sequence: online (one push, one advance) against upload + prefilter + init_pass
    x0 = odo[:, 0]
    for _ in range(2):   # (the second round is reported)
        a = _now()
        eng.online_begin(zz.shape[0], capacity=T)
        eng.online_push(zz, odo, u)
        b = _now()
        eng.online_advance()
        c = _now()
        eng.online_finish()
        d = _now()
        st = eng.online_state()
        ref = SweepEngine(cfg)
        e = _now()
        ref.upload(zz, odo, u)
        f = _now()
        x, y, cnt, lact, _ = ref.init_pass(x0)
        g = _now()
        ref.close()
    out["whole_ms"] = {"online_push": round(b - a, 3), "online_advance": round(c - b, 3),
                       "upload_prefilter": round(f - e, 3), "init_pass": round(g - f, 3),
                       "identical": bool(np.array_equal(st[0], x) and np.array_equal(st[1], y) and st[3] == lact)}
    out["finish_ms"] = {"online_finish": round(d - c, 3), "upload_prefilter": round(f - e, 3)}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"tool": "online_latency"}
    d = np.load(os.path.join(ROOT, "tests", "golden", "data_IJAC2018.npz"))
    cfg = ConfigICM("config_default.yaml")
    z = d["observations"]
    zz = np.ascontiguousarray(np.minimum(z + cfg.radio, z * 0.0 + cfg.rango_laser_max))
    res["dataset"] = _stream(cfg, zz, np.ascontiguousarray(d["odometry"]), np.ascontiguousarray(d["velocities"]))
    wl = make_workload(args.samples, 1000, 360)
    res["synthetic"] = _stream(ConfigICM(D=dict(wl.config, L=args.samples + 5000)), np.ascontiguousarray(wl.scans.T), wl.odometry, wl.u)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
