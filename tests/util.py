"""Shared helpers of the test-suite: golden fixtures, configs."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def gold(name):
    return np.load(os.path.join(GOLD, name))


class Cfg:
    """The numeric options of config_ros.yaml / config_default.yaml (identical values)."""

    def __init__(self, **kw):
        self.N = 2
        self.deltat = 0.1
        self.L = 1000
        self.Q = np.eye(2)
        self.R = np.eye(3)
        self.cte_odom = 1.0
        self.cota = 300.0
        self.dist_thr = 1.0
        self.dist_thr_obs = 1.0
        self.rango_laser_max = 10.0
        self.radio = 0.137
        self.angle_increment = None
        for k, v in kw.items():
            setattr(self, k, v)


def dataset():
    """(zz (181,1833) prepared ranges, odometry (3,T), velocities (2,T)) of data_IJAC2018."""
    d = gold("data_IJAC2018.npz")
    z = d["observations"]
    cfg = Cfg()
    zz = np.minimum(z + cfg.radio, z * 0 + cfg.rango_laser_max)  # scripts/sensors_definitions.py:22
    return zz, d["odometry"], d["velocities"]


def label_digest(off, labels):
    """One 64-bit word per pose from the labels of its kept beams (order-sensitive, wrap-around
    arithmetic): sum_j (label_j + 2) * (j * 2654435761 + 0x9E3779B1) over the pose's beams j = 0..n-1.
    Full-size fixtures keep this instead of the 23 M labels themselves."""
    off = np.asarray(off, dtype=np.int64)
    lab = np.asarray(labels).astype(np.int64).astype(np.uint64)
    n = off[1:] - off[:-1]
    if lab.size == 0:
        return np.zeros(n.size, dtype=np.uint64)
    j = (np.arange(lab.size, dtype=np.int64) - np.repeat(off[:-1], n)).astype(np.uint64)
    with np.errstate(over="ignore"):
        w = (lab + np.uint64(2)) * (j * np.uint64(2654435761) + np.uint64(0x9E3779B1))
        h = np.add.reduceat(w, np.minimum(off[:-1], lab.size - 1))
    h[n == 0] = 0
    return h


def hip_runtime():
    """ctypes handle of the HIP runtime this process ALREADY has loaded (the copy libicmslam_hip.so is bound to: the
    PyTorch wheel's or the system's) -- found by its path in /proc/self/maps, never by a bare name that could pull a
    second runtime into the process."""
    import ctypes
    for ln in open("/proc/self/maps"):
        path = ln.split()[-1]
        if "libamdhip64.so" in path and os.path.exists(path):
            return ctypes.CDLL(path)
    raise RuntimeError("no HIP runtime loaded in this process yet")


def check_runs(eng, thr):
    """Structure of the runs: a partition of every pose's kept beams into consecutive stretches, cut by the stated rule,
    with a bounding circle that really bounds and the sum that really is the sum."""
    off, bk, d, bx, by = eng.kept_beams()
    roff, c, sb, r, k, f = eng.runs()
    n_runs, _ = eng.run_counts()
    assert roff[0] == 0 and roff[-1] == n_runs == len(k)
    nb = np.diff(off)
    pose_of_run = np.repeat(np.arange(len(nb)), np.diff(roff))
    assert np.array_equal(np.bincount(pose_of_run, weights=k, minlength=len(nb)).astype(np.int64), nb), "the runs of a pose hold all its beams"
    # consecutive: the first run starts at the pose's first beam, each next one where the last ended
    first_of_pose = roff[:-1][np.diff(roff) > 0]
    assert not f[first_of_pose].any()
    same = pose_of_run[1:] == pose_of_run[:-1]
    assert np.array_equal((f[:-1] + k[:-1])[same], f[1:][same])
    assert k.min() >= 1 and k.max() <= 64   # (kRunCap)
    start = off[pose_of_run] + f                    # absolute index of each run's first beam
    run_of_beam = np.repeat(np.arange(n_runs), k)   # (runs are in beam order)
    assert np.array_equal(np.repeat(start, k) + (np.arange(len(run_of_beam)) - np.repeat(np.cumsum(k) - k, k)), np.arange(len(bx)))
    # the sum and the circle
    sx = np.bincount(run_of_beam, weights=bx, minlength=n_runs)
    sy = np.bincount(run_of_beam, weights=by, minlength=n_runs)
    assert np.abs(sb[:, 0] - sx).max() <= 1e-12 * max(1.0, np.abs(sx).max()) and np.abs(sb[:, 1] - sy).max() <= 1e-12 * max(1.0, np.abs(sy).max())
    dist = np.hypot(bx - c[run_of_beam, 0], by - c[run_of_beam, 1])
    assert (dist <= r[run_of_beam].astype(np.float64)).all(), "every beam inside its run's circle"
    assert np.abs(c[:, 0] - sx / k).max() <= 1e-12 and np.abs(c[:, 1] - sy / k).max() <= 1e-12
    # the cutting rule: inside a run, neighbours within the gap and everybody within the extent of the first beam
    gap, ext = 0.35 * thr, 0.5 * thr
    inner = np.ones(len(bx), dtype=bool)
    inner[start] = False
    j = np.flatnonzero(inner)
    assert (np.hypot(bx[j] - bx[j - 1], by[j] - by[j - 1]) <= gap * (1 + 1e-12)).all()
    assert (np.hypot(bx - bx[start][run_of_beam], by - by[start][run_of_beam]) <= ext * (1 + 1e-12)).all()
    # ... and a run begins only where the rule asks for it
    heads = start[f > 0]
    prev_start = start[np.flatnonzero(f > 0) - 1]
    g_ = np.hypot(bx[heads] - bx[heads - 1], by[heads] - by[heads - 1])
    e_ = np.hypot(bx[heads] - bx[prev_start], by[heads] - by[prev_start])
    full = k[np.flatnonzero(f > 0) - 1] == 64
    assert ((g_ > gap * (1 - 1e-12)) | (e_ > ext * (1 - 1e-12)) | full).all()
    return n_runs, float(k.mean()), float(r.max())


def entry_layout(nloc):
    """The host's layout of the hierarchical entry pipeline for a shard of nloc poses (icm_prefilter; kMaxSuper = 64
    matrix rows): poses per chunk, chunks per superchunk, superchunks, chunks."""
    ch = 64 if nloc >= 65536 else (32 if nloc >= 16384 else 16)
    nchunks = (nloc + ch - 1) // ch
    g = (nchunks + 63) // 64
    return dict(chunk_poses=ch, chunk_group=g, nsuper=(nchunks + g - 1) // g, nchunks=nchunks)
