"""Wide scans for the suite (host only, deterministic): scenes whose scans reach past the first 64 beams, runs and entries
that every per-scan kernel handles one wave at a time -- full-length runs (k = kRunCap = 64), more than 64 and more than
128 runs per scan, 97-192 labels per scan, scans with no kept beam between wide ones -- at B up to ICM_MAX_BEAMS.

The robot turns on the spot at the origin (u = [0, w]), so every scan is known in advance: the range of a beam depends on
its index only, not on the heading, and the runs of a scan (oracle.cut_runs: cut at 0.35 / 0.5 dist_thr and after 64
beams) follow from the scene's geometry alone.  What the heading and the map change is the association.

  ring    a circle of returns RING_R = 3 m from the sensor (B >= 360; 1.5 m for smaller B), seen in whole or by its first
          `nb` beams, with landmarks every 0.4 m on it, a twin 0.06 m beside a third of them and crowds of five around a
          few (runs the bounding-circle test cannot settle, in every batch of 64 runs), and a near arc: beams
          0..ARC_BEAMS-1 of a "full" scan return from ARC_R = 0.3 m, where 64 consecutive beams span less than 0.5
          dist_thr -- runs cut by the cap.  At B = 1440 consecutive ring beams are 0.0131 m apart, so a run holds 8 of
          them: a ring of nb = 8 n beams is exactly n runs.  <= 96 labels per scan (the 128-slot table, no relaunch).
  dense   the same ring with landmarks every 0.12 m and no clutter: 97-192 labels per full scan (the 256-slot relaunch
          with multi-beam runs, more than 64 entries per pose).
  trunks  trunks of radius 0.05 m every 0.4 m on the 3 m circle and nothing in between: 7-8 beams per trunk, ~360 kept
          beams per scan, one cluster per trunk in the first scan -- the initialisation pass's input.

build() returns a Scene with what SweepEngine.upload and the oracles take; reach() measures, with the NumPy oracle, what a
scene reaches in sweep 1 (from the scene's map and x_init) and the smallest distance of any run to the three margins of
the bounding-circle test.  The oracle decides in double, the kernel in single precision: only when no run lies within
MARGIN_TOL * dist_thr of a margin must their counts of unsettled runs agree, so build() redraws the map's jitter until
none does.
"""
import numpy as np

from oracle import icm_oracle as o

RING_R = 3.0
SMALL_RING_R = 1.5         # B < 360: 0.147 m between beams at B = 64 (kept at dist_thr 0.2, one beam per run)
ARC_R = 0.3
ARC_BEAMS = 360
RMAX = 10.0
THR = 0.2
MARGIN_TOL = 1e-5          # of dist_thr
W = 0.05                   # turn rate [rad/s]: 0.005 rad per pose
DT = 0.1

# what pose t's scan is, by t mod the pattern: "full" = near arc + ring, "ring" = the whole ring, ("ring", nb) = its
# first nb beams, "empty" = nothing in range.  At B = 1440: 141 / 180 runs, 63 / 64 / 65 / 128 / 129 runs, 63 / 64 /
# 65 / 128 / 129 kept beams.
WIDE_KINDS = ["full", ("ring", 504), ("ring", 512), "empty", ("ring", 520), "ring", ("ring", 1024), ("ring", 1032),
              ("ring", 63), ("ring", 64), ("ring", 65), "empty", ("ring", 128), ("ring", 129), "full", "ring"]


def small_kinds(B):
    # (a ring of nb < B beams keeps nb of them -- the 3-tap median pads with zeros, so nb = B - 1 would keep B)
    return ["ring", ("ring", B - 2), "empty", ("ring", B // 2 + 1)]


class Scene:
    pass


def config(B, thr=THR, L=None):
    """ConfigICM values of a scene (angle_increment = 2 pi / B: a full circle)."""
    return dict(N=1, deltat=DT, L=int(L), Q=[1.0, 1.0], R=[1.0, 1.0, 1.0], cte_odom=1.0, cota=1.0, dist_thr=thr,
                dist_thr_obs=1.0, rango_laser_max=RMAX, radio=0.0, angle_increment=2 * np.pi / B)


def _on_circle(r, spacing, phase=0.0):
    n = max(int(round(2 * np.pi * r / spacing)), 1)
    a = phase + 2 * np.pi * np.arange(n) / n
    return r * np.stack((np.cos(a), np.sin(a)))


def _trunk_ranges(B, heading, centres, rho):
    """Ranges from the origin to circles of radius rho around `centres` (2,n), beam b at world angle heading - pi/2 +
    b 2 pi / B; RMAX where no circle is hit."""
    a = heading - np.pi / 2 + 2 * np.pi * np.arange(B) / B
    ux, uy = np.cos(a)[:, None], np.sin(a)[:, None]
    p = ux * centres[0][None, :] + uy * centres[1][None, :]           # along the ray
    q2 = (centres ** 2).sum(axis=0)[None, :] - p * p                  # squared distance of the centre from the ray
    hit = (p > 0) & (q2 < rho * rho)
    s = np.where(hit, p - np.sqrt(np.maximum(rho * rho - q2, 0.0)), np.inf).min(axis=1)
    return np.where(np.isfinite(s), s, RMAX)


def build(kind="ring", B=1440, T=96, seed=0, wide_at=()):
    """A Scene: ranges (B,T) beam-major like the reference's `mediciones`, odometry (3,T), u (2,T), map (2,K), x_init
    (3,T), x0 (3,), config (dict), kinds (T,) and reach (dict, see reach()).  Poses in `wide_at` and the last pose see
    the whole ring."""
    rng = np.random.default_rng(seed)
    small = B < ARC_BEAMS
    ring_r = SMALL_RING_R if small else RING_R
    kinds = small_kinds(B) if small else WIDE_KINDS
    per_pose = [kinds[t % len(kinds)] for t in range(T)]
    for t in list(wide_at) + [T - 1]:
        per_pose[t] = "ring"
    heading = np.pi / 2 + W * DT * np.arange(T)
    x_true = np.stack((np.zeros(T), np.zeros(T), heading))
    u = np.stack((np.zeros(T), np.full(T, W)))
    ranges = np.full((B, T), RMAX)
    noise = rng.normal(0.0, 1e-3, (B, T))
    if kind == "trunks":
        trunks = _on_circle(RING_R, 0.4)
        for t in range(T):
            ranges[:, t] = _trunk_ranges(B, heading[t], trunks, 0.05)
            if per_pose[t] == "empty":
                ranges[:, t] = RMAX
            elif isinstance(per_pose[t], tuple):
                ranges[per_pose[t][1]:, t] = RMAX
        ranges = np.where(ranges < RMAX, ranges + 0.2 * noise, RMAX)
        base = trunks
    else:
        for t, kd in enumerate(per_pose):
            if kd == "empty":
                continue
            nb = B if kd in ("full", "ring") else min(kd[1], B)
            ranges[:nb, t] = ring_r + noise[:nb, t]
            if kd == "full" and not small:
                ranges[:ARC_BEAMS, t] = ARC_R + 0.1 * noise[:ARC_BEAMS, t]
        if kind == "ring":
            base = _on_circle(ring_r, 0.4)
            extra = [_on_circle(ARC_R, 0.3, 0.2)] if not small else []
            twins_of = base[:, ::3]
            v = rng.normal(0.0, 1.0, twins_of.shape)
            extra.append(twins_of + 0.06 * v / np.linalg.norm(v, axis=0))
            for i in rng.choice(base.shape[1], 3, replace=False):
                a = 2 * np.pi * np.arange(5) / 5 + rng.uniform(0, 1)
                extra.append(base[:, [i]] + 0.08 * np.stack((np.cos(a), np.sin(a))))
            base = np.concatenate([base] + extra, axis=1)
        elif kind == "dense":
            base = _on_circle(ring_r, 0.12)
            if not small:
                base = np.concatenate((base, _on_circle(ARC_R, 0.3, 0.2)), axis=1)
        else:
            raise ValueError(kind)
    x_init = x_true + np.stack((rng.normal(0, 0.01, T), rng.normal(0, 0.01, T), rng.normal(0, 0.002, T)))
    x_init[:, 0] = x_true[:, 0]
    sc = Scene()
    sc.kind, sc.B, sc.T, sc.seed = kind, B, T, seed
    sc.ranges, sc.u, sc.odometry, sc.x_true = ranges, u, x_true.copy(), x_true
    sc.x_init, sc.x0 = x_init, x_init[:, 0].copy()
    sc.kinds = per_pose
    sc.thr = THR
    sc.config = config(B, THR, L=base.shape[1] + 4096)
    # the map: the landmarks jittered by 0.01 m, redrawn until no run of sweep 1 lies within MARGIN_TOL * dist_thr of a
    # margin of the bounding-circle test (at most a few runs in 10^4 do for a given draw)
    for attempt in range(20):
        sc.map = base + np.random.default_rng((seed, attempt)).normal(0.0, 0.01, base.shape)
        sc.reach = reach(sc)
        if sc.reach["min_margin"] > MARGIN_TOL * THR:
            return sc
    raise RuntimeError("no map draw keeps every run off the margins of the bounding-circle test")


def oracle_config(sc):
    return o.OracleConfig(deltat=DT, L=sc.config["L"], cota=sc.config["cota"], dist_thr=sc.thr, rango_laser_max=RMAX,
                          radio=0.0, angle_increment=sc.config["angle_increment"])


def run_circle(body):
    """Centre (2,) and radius of the bounding circle a run's record carries (k_run_build's construction, in double)."""
    c = body.sum(axis=0) / body.shape[0]
    return c, np.sqrt(((body - c) ** 2).sum(axis=1)).max() * 1.000001 + 1e-12


def margins(centre_w, radius, ref_map, lact, thr):
    """Signed slack of the three inequalities of oracle.run_decision for one run (inf where a test does not apply: no
    or more than four candidates, no second candidate)."""
    K = min(int(lact), ref_map.shape[1])
    mx, my = ref_map[0, :K], ref_map[1, :K]
    cell = thr * (1.0 + 1e-9)
    gx0, gy0 = mx.min(), my.min()
    nx, ny = int(np.floor((mx.max() - gx0) / cell)) + 1, int(np.floor((my.max() - gy0) / cell)) + 1
    cx = int(np.clip(np.floor((centre_w[0] - gx0) / cell), 0, nx - 1))
    cy = int(np.clip(np.floor((centre_w[1] - gy0) / cell), 0, ny - 1))
    lx = np.clip(np.floor((mx - gx0) / cell), 0, nx - 1)
    ly = np.clip(np.floor((my - gy0) / cell), 0, ny - 1)
    cand = np.flatnonzero((np.abs(lx - cx) <= 1) & (np.abs(ly - cy) <= 1))
    if cand.size == 0 or cand.size > 4:
        return np.inf, np.inf, np.inf
    d = np.sort(np.sqrt((mx[cand] - centre_w[0]) ** 2 + (my[cand] - centre_w[1]) ** 2))
    eps, r = 1e-4 * thr, float(radius)
    m1 = (thr - eps) - (d[0] + r)
    m2 = cell * (1.0 - 1e-4) - (d[0] + 2 * r)
    m3 = (d[1] - d[0]) - (2 * r + eps) if d.size > 1 else np.inf
    return m1, m2, m3


def reach(sc, x=None, ref_map=None):
    """What sweep 1 of the scene reaches, by the NumPy oracle: per pose kept beams, runs, capped runs (k = 64), labels
    (distinct values of the reference's `c`, the fresh one included), whether a fresh label is made, and the runs the
    bounding-circle test does not settle by batch of 64 runs; min_margin = the smallest |slack| of any run."""
    cfg = oracle_config(sc)
    x = sc.x_init if x is None else x
    ref_map = sc.map if ref_map is None else ref_map
    K = ref_map.shape[1]
    kept = o.prefilter_all(sc.ranges, cfg)
    out = dict(kept=[], runs=[], capped=0, labels=[], fresh=[], unsettled=0, unsettled_batch=[0, 0, 0],
               settled_batch=[0, 0, 0], min_margin=np.inf, multi_beam_runs=[])
    for t, kz in enumerate(kept):
        n = kz.shape[0] if kz.ndim == 2 else 0
        out["kept"].append(n)
        if n == 0:
            out["runs"].append(0), out["labels"].append(0), out["fresh"].append(False), out["multi_beam_runs"].append(0)
            continue
        body = kz[:, 2:4]
        pose = sc.x0 if t == 0 else x[:, t]
        lab = o.associate(ref_map, K, o.project_beams(pose, body), sc.thr)
        out["labels"].append(len(np.unique(lab)))
        out["fresh"].append(bool((lab == -1).any()))
        runs = o.cut_runs(body, sc.thr)
        out["runs"].append(len(runs))
        out["multi_beam_runs"].append(sum(k > 1 for _, k in runs))
        out["capped"] += sum(k == o.RUN_CAP for _, k in runs)
        for q, (first, k) in enumerate(runs):
            c, r = run_circle(body[first:first + k])
            cw = o.project_beams(pose, c[None, :])[0]
            out["min_margin"] = min(out["min_margin"], *(abs(m) for m in margins(cw, r, ref_map, K, sc.thr)))
            if o.run_decision(cw, r, ref_map, K, sc.thr) is None:
                out["unsettled"] += 1
                out["unsettled_batch"][min(q // 64, 2)] += 1
            elif k > 1:
                out["settled_batch"][min(q // 64, 2)] += 1
    return out


def summary(sc):
    r = sc.reach
    return ("%s B=%d T=%d: capped runs %d, most runs per pose %d, most kept beams per pose %d, labels per pose <= %d, "
            "unsettled runs %d (batch 0/1/2+: %s), settled multi-beam runs by batch %s, min margin %.1e m"
            % (sc.kind, sc.B, sc.T, r["capped"], max(r["runs"]), max(r["kept"]), max(r["labels"]), r["unsettled"],
               "/".join(map(str, r["unsettled_batch"])), "/".join(map(str, r["settled_batch"])), r["min_margin"]))


_CACHE = {}


def scene(kind="ring", B=1440):
    """The suite's scenes, built once per process: 96 poses at B >= 360, 40 below."""
    key = (kind, B)
    if key not in _CACHE:
        _CACHE[key] = build(kind, B, 96 if B >= ARC_BEAMS else 40, wide_at=GHOSTS_96 if B >= ARC_BEAMS else ())
    return _CACHE[key]


def shard_ghosts(T, worlds=(2, 3)):
    """Ghost poses (the pose in front of each shard but the first) of a T-pose sequence split `world` ways (contiguous
    blocks of ceil(T / world) poses rounded up to an even number, icm_shard_block)."""
    out = set()
    for w in worlds:
        blk = (T + w - 1) // w
        blk += blk & 1
        out.update(r * blk - 1 for r in range(1, w) if r * blk < T)
    return tuple(sorted(out))


GHOSTS_96 = shard_ghosts(96)
