"""Scenes for phase B's layout and table limits (host only, deterministic, seeded): how many distinct labels each pose,
chunk and superchunk of the hierarchical entry pipeline sees, and where the poses that create a landmark lie.

The conveyor: a robot drives the x axis (heading 0) through a band of trunks on both sides of a free corridor, ray-cast
with icmslam_hip.synthetic.raycast.  Its speed is set per pose (negative = reversing, so a long sequence can shuttle
over the same stretch and keep its coordinates small), and the laser range RANGE = 3 m bounds what one pose sees:
  * a sparse band (pitch SPARSE) gives ~10 labels per pose, whatever the chunking;
  * a dense patch (pitch DENSE) driven through fast gives one chunk or one superchunk ~200 or ~1500 distinct labels;
  * clutter poses: three beams straight ahead return from 1.5 m, in the trunk-free corridor, farther than dist_thr from
    every landmark.  Each such pose creates one fresh landmark of 3 observations in every sweep (cota = 5 prunes it
    again), so it adds exactly one distinct label to its chunk and superchunk -- the fine adjustment to an exact count.

util.entry_layout mirrors the host's layout (icm_prefilter) and reach() measures, from the C oracle's labels of
sweep 1, what a scene reaches; expected_path() is the pipeline the sweep must run (the rule of k_chunk_l1 / k_chunk_l2).
"""
import numpy as np

from icmslam_hip import synthetic as syn
from util import entry_layout

RANGE = 3.0          # rango_laser_max [m]
THR = 0.3            # dist_thr: below the corridor's half-width and half the densest pitch
CORRIDOR = 0.6       # no trunk centre within this distance of the path
BAND = 2.6           # trunk centres up to this distance from the path
SPARSE = 1.5
DENSE = 0.62
CLUTTER_R = 1.5
DT = 0.1
COTA = 5.0

WAVE = 64            # kWave: entries per pose
CHUNK_CAP = 256 - 32  # kT1 - 32
SUPER_CAP = 1536     # kT2Cap


class Scene:
    pass


def band(x0, x1, pitch, rng):
    """Trunk centres (2,n) on a jittered grid of `pitch` over x in [x0, x1), CORRIDOR <= |y| <= BAND."""
    xs = np.arange(x0, x1, pitch)
    ys = np.arange(CORRIDOR + 0.1, BAND, pitch)
    ys = np.concatenate((ys, -ys))
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    pts = np.stack((gx.ravel(), gy.ravel()))
    j = 0.15 * pitch
    pts = pts + rng.uniform(-j, j, pts.shape)
    pts[1] = np.sign(pts[1]) * np.clip(np.abs(pts[1]), CORRIDOR, BAND)
    return pts


def config(B, L):
    return dict(N=1, deltat=DT, L=int(L), Q=[1.0, 1.0], R=[1.0, 1.0, 1.0], cte_odom=1.0, cota=COTA, dist_thr=THR,
                dist_thr_obs=1.0, rango_laser_max=RANGE, radio=syn.RADIO, angle_increment=2 * np.pi / B)


def path(speed):
    """x positions of the poses driving at speed[t] [m per pose] from x = 0."""
    return np.concatenate(([0.0], np.cumsum(speed[:-1])))


def shuttle(T, v, length):
    """Per-pose speeds: back and forth over `length` metres at v per pose."""
    n = max(int(round(length / v)), 1)
    s = np.where((np.arange(T) // n) % 2 == 0, v, -v)
    return s


def make(T, speed, trunks, clutter=(), B=180, seed=0, label=""):
    """A Scene: ranges (B,T) beam-major, odometry / x_true / x_init (3,T), u (2,T), map (2,K), x0, config."""
    rng = np.random.default_rng(seed)
    speed = np.asarray(speed, dtype=np.float64)
    xs = path(speed)
    x_true = np.stack((xs, np.zeros(T), np.zeros(T)))
    u = np.stack((speed / DT, np.zeros(T)))
    inc = 2 * np.pi / B
    z = syn.raycast(x_true, trunks, B, inc, rng.normal(0.0, 1e-3, (T, B)))
    z = np.minimum(z + syn.RADIO, syn.RMAX)
    clutter = np.asarray(sorted(set(int(t) for t in clutter)), dtype=np.int64)
    ahead = B // 4                     # sensor bearing pi/2 = straight ahead
    for d in (-1, 0, 1):
        z[clutter, ahead + d] = CLUTTER_R
    x_init = x_true + np.stack((rng.normal(0, 0.01, T), rng.normal(0, 0.01, T), rng.normal(0, 0.002, T)))
    x_init[:, 0] = x_true[:, 0]
    sc = Scene()
    sc.label, sc.T, sc.B, sc.seed = label, T, B, seed
    sc.ranges = np.ascontiguousarray(z.T)
    sc.u, sc.odometry, sc.x_true, sc.x_init, sc.x0 = u, x_true.copy(), x_true, x_init, x_init[:, 0].copy()
    sc.trunks = trunks
    sc.map = trunks + np.random.default_rng((seed, 1)).normal(0.0, 0.01, trunks.shape)
    sc.clutter = clutter
    sc.config = config(B, trunks.shape[1] + 4096 + clutter.size)
    return sc


def cfg_of(sc):
    from ICM_SLAM_tools import ConfigICM
    return ConfigICM(D=sc.config)


# ---- labels --------------------------------------------------------------------------------------------------------
def labels_c(sc, x=None, mapa=None):
    """Sweep 1's labels by the C oracle: (off (T+1,), labels (nnz,)); fresh labels are lact0 + rank."""
    from oracle import c_oracle as co
    cfg = cfg_of(sc)
    kept = co.prefilter(cfg, sc.ranges)
    x = (sc.x_init if x is None else x).copy()
    mapa = sc.map if mapa is None else mapa
    a = {}
    co.sweep(cfg, kept, sc.u, sc.odometry, sc.x0, mapa, x, mapa.shape[1], "redblack", assoc=a)
    return kept[0], a["labels"]


def labels_window(sc, poses):
    """Labels of the given poses by the NumPy oracle (filtrar_z, associate against the landmarks within reach -- the
    same nearest one), one fresh label per pose that has a gated-out beam: {t: set of labels}."""
    from oracle import icm_oracle as o
    cfg = o.OracleConfig(deltat=DT, L=sc.config["L"], cota=COTA, dist_thr=THR, rango_laser_max=RANGE, radio=0.0,
                         angle_increment=sc.config["angle_increment"])
    K = sc.map.shape[1]
    out = {}
    for t in poses:
        kz = o.filtrar_z(sc.ranges[:, t], cfg)
        if kz.ndim != 2 or kz.shape[0] == 0:
            out[t] = set()
            continue
        px, py = sc.x_init[:2, t]
        w = o.project_beams(sc.x_init[:, t], kz[:, 2:4])
        wx, wy = w[:, 0], w[:, 1]
        near = np.flatnonzero(np.hypot(sc.map[0] - px, sc.map[1] - py) < RANGE + 2 * THR + 1.0)
        if near.size == 0:
            lab = np.full(wx.size, -1)
        else:
            d = np.hypot(sc.map[0, near][None, :] - wx[:, None], sc.map[1, near][None, :] - wy[:, None])
            lab = near[np.argmin(d, axis=1)]
            lab[d.min(axis=1) > THR] = -1
        out[t] = set(int(v) for v in lab[lab >= 0]) | ({K + t} if (lab < 0).any() else set())
    return out


# ---- what a scene reaches ------------------------------------------------------------------------------------------
def reach(sc, off=None, labels=None):
    """Per pose entries (distinct labels), per chunk and per superchunk distinct labels (fresh ones included) under the
    host's layout, and the chunks of the poses that create a landmark -- from the C oracle's labels of sweep 1."""
    if labels is None:
        off, labels = labels_c(sc)
    K = sc.map.shape[1]
    lay = entry_layout(sc.T)
    CH, G = lay["chunk_poses"], lay["chunk_group"]
    T = sc.T
    n = np.diff(off)
    pose = np.repeat(np.arange(T), n)
    lab = np.asarray(labels, dtype=np.int64)
    # (pose, label) pairs = entries
    key = np.unique(pose * (1 << 32) + lab)
    ep, el = key >> 32, key & 0xFFFFFFFF
    entries = np.bincount(ep, minlength=T)
    ck = np.unique((ep // CH) * (1 << 32) + el)
    per_chunk = np.bincount(ck >> 32, minlength=lay["nchunks"])
    sk = np.unique((ep // (CH * G)) * (1 << 32) + el)
    per_super = np.bincount(sk >> 32, minlength=lay["nsuper"])
    creators = np.unique(ep[el >= K])
    return dict(layout=lay, entries=entries, per_chunk=per_chunk, per_super=per_super, creators=creators,
                creator_chunks=np.unique(creators // CH), last_chunk_poses=T - (lay["nchunks"] - 1) * CH)


def expected_path(r):
    if r["entries"].max() > WAVE or r["per_chunk"].max() > CHUNK_CAP or r["per_super"].max() > SUPER_CAP:
        return "sort"
    return "hier"


# ---- tuning to an exact count --------------------------------------------------------------------------------------
def _unit_count(sc, poses):
    labs = labels_window(sc, poses)
    return len(set().union(*labs.values())), labs


def _tune(build, poses, target, lo_pad):
    """build(m, clutter) -> Scene with the first m patch trunks and clutter poses; finds m whose unit count (distinct
    labels over `poses`) lies in [target - lo_pad, target], then pads with clutter poses (one fresh label each) on
    poses of the unit that create none yet."""
    lo, hi = 0, None
    m = 64
    for _ in range(40):
        sc = build(m, ())
        cnt, labs = _unit_count(sc, poses)
        if target - lo_pad <= cnt <= target:
            break
        if cnt > target:
            hi = m
        else:
            lo = m
        m = (lo + hi) // 2 if hi is not None else 2 * m
    else:
        raise RuntimeError("no patch size reaches %d" % target)
    K = sc.map.shape[1]
    free = [t for t in poses if K + t not in labs[t] and len(labs[t]) < WAVE]
    need = target - cnt
    clutter = free[len(free) // 2 - need // 2:][:need] if need else []
    sc = build(m, clutter)
    cnt2, _ = _unit_count(sc, poses)
    if cnt2 != target:
        raise RuntimeError("clutter padding reached %d, not %d" % (cnt2, target))
    return sc


# ---- the scenes ----------------------------------------------------------------------------------------------------
def layout_scene(T, B=180, seed=0, clutter=(), label=""):
    """Sparse shuttle over 40 m at 0.2 m per pose: a few labels per pose, coordinates within 45 m."""
    speed = shuttle(T, 0.2, 40.0)
    xs = path(speed)
    rng = np.random.default_rng((seed, 7))
    trunks = band(xs.min() - RANGE - 1, xs.max() + RANGE + 1, SPARSE, rng)
    return make(T, speed, trunks, clutter, B, seed, label)


def ranks_scene(T=33000, seed=0):
    """Fresh landmarks in chunk 0, in chunks beyond 512 (CH 32) and in the last chunk, in every sweep."""
    lay = entry_layout(T)
    CH, nch = lay["chunk_poses"], lay["nchunks"]
    cl = [1, 5] + [c * CH + 3 for c in (513, 600, 777, 1000)] + [c * CH + 11 for c in (700,)] + [(nch - 1) * CH + 2, T - 1 - 1]
    return layout_scene(T, seed=seed, clutter=cl, label="ranks")


def _limit_scene(T, unit, j, target, seed, label):
    """A sparse line at 0.05 m per pose with a dense patch (in place of the sparse band) driven through fast by the poses of chunk or superchunk j
    (unit = 'chunk' / 'super'), tuned to `target` distinct labels there."""
    lay = entry_layout(T)
    CH, G = lay["chunk_poses"], lay["chunk_group"]
    n_unit = CH if unit == "chunk" else CH * G
    t0 = j * n_unit
    poses = list(range(t0, t0 + n_unit))
    vf = 24.0 / CH if unit == "chunk" else 1.0       # chunk: 24 m; superchunk: one metre per pose
    speed = np.full(T, 0.05)
    speed[t0:t0 + n_unit] = vf
    xs = path(speed)
    rng = np.random.default_rng((seed, 11))
    base = band(xs.min() - RANGE - 1, xs.max() + RANGE + 1, SPARSE, rng)
    # patch: dense trunks over the unit's stretch, away from the sparse ones, in a seeded order; the first m are kept
    px0, px1 = xs[t0], xs[t0 + n_unit - 1]
    base = base[:, (base[0] < px0 - DENSE) | (base[0] >= px1 + DENSE)]
    patch = band(px0, px1, DENSE, np.random.default_rng((seed, 12)))
    patch = patch[:, np.random.default_rng((seed, 13)).permutation(patch.shape[1])]

    def build(m, clutter):
        sc = make(T, speed, np.concatenate((base, patch[:, :min(m, patch.shape[1])]), axis=1), clutter, 360, seed, label)
        sc.n_base = base.shape[1]      # map columns [0, n_base) = the sparse band
        return sc

    lo_pad = min(12, n_unit // 2)
    return _tune(build, poses, target, lo_pad)


_CACHE = {}


def scene(name):
    """Named scenes (cached per process)."""
    if name in _CACHE:
        return _CACHE[name]
    kind, _, arg = name.partition(":")
    if kind == "layout":
        sc = layout_scene(int(arg), label=name)
    elif kind == "ranks":
        sc = ranks_scene()
        sc.label = name
    elif kind in ("chunk224", "chunk225"):
        T = int(arg)                   # 2048: CH 16; 16384: CH 32
        lay = entry_layout(T)
        sc = _limit_scene(T, "chunk", lay["nchunks"] // 2 + 1, int(kind[5:]), 0, name)
    elif kind in ("super1536", "super1537"):
        T = int(arg)                   # 16383: CH 16, G 16
        lay = entry_layout(T)
        sc = _limit_scene(T, "super", lay["nsuper"] // 2, int(kind[5:]), 0, name)
    else:
        raise KeyError(name)
    _CACHE[name] = sc
    return sc


LAYOUT = ["layout:1024", "layout:4096", "layout:1025", "layout:16383", "layout:16384", "layout:40001", "layout:65535",
          "layout:65536"]
LIMITS = ["chunk224:2048", "chunk225:2048", "chunk224:16384", "chunk225:16384", "super1536:16383", "super1537:16383"]
