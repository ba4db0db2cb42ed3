"""Phase B -- the hierarchical entry pipeline (k_chunk_l1<16/32/64>, k_chunk_l2, k_lm_l3, k_rec_push, the moment
targets) -- at every chunk size and at the edges of its layout and its tables (tests/phase_b_shapes.py):

layout        icm_get_entry_layout == the host formula's mirror (util.entry_layout) for every size used here
targets       labels == the C oracle's; per-beam targets within 1e-11 m of running means formed in np.longdouble from the
              labels, the poses before the sweep and the kept beams, and within 1e-12 of the sort-based pipeline's
sweep         one sweep against the C oracle: K, counts exact; raw map, map and poses <= 1e-9
fallback      the pipeline a sweep runs == expected_path(labels): > 64 entries per pose, > 224 distinct labels per chunk
              or > 1536 per superchunk, through sweep() and through a sweep queued whole; sticky until set_state
ranks         sweeps queued whole without the scan kernels rank new landmarks beyond chunk 512 right
shards        virtual ranks whose chunking differs from the unsharded run's equal it
"""
import os

import numpy as np
import pytest

import phase_b_shapes as pb
from util import entry_layout

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(autouse=True, scope="module")
def _threads():
    from oracle import c_oracle as co
    co.set_threads(min(16, int(os.environ.get("OMP_NUM_THREADS", "8") or 8)))


def _engine(sc, **kw):
    from icmslam_hip import SweepEngine
    eng = SweepEngine(pb.cfg_of(sc))
    eng.upload(sc.ranges, sc.odometry, sc.u, **kw)
    return eng


def _oracle_sweep(sc, x, mapa, lact, schedule="redblack"):
    from oracle import c_oracle as co
    cfg = pb.cfg_of(sc)
    kept = co.prefilter(cfg, sc.ranges)
    a = {}
    m, cnt, K, raw = co.sweep(cfg, kept, sc.u, sc.odometry, sc.x0, mapa, x, lact, schedule, assoc=a)
    return m, cnt, K, raw, a["labels"], kept[0]


def _ref_targets(off, bx, by, lab, x):
    """Per kept beam: the running mean, in time, of its landmark's world points through its pose -- np.longdouble."""
    T = x.shape[1]
    n = np.diff(off)
    pose = np.repeat(np.arange(T), n)
    th = x[2].astype(np.longdouble)[pose] - np.longdouble(np.pi) / 2     # (oracle.project_beams' frame)
    ct, st = np.cos(th), np.sin(th)
    bxl, byl = bx.astype(np.longdouble), by.astype(np.longdouble)
    wx = bxl * ct - byl * st + x[0].astype(np.longdouble)[pose]
    wy = bxl * st + byl * ct + x[1].astype(np.longdouble)[pose]
    lab = lab.astype(np.int64)
    key = lab * T + pose
    order = np.argsort(key, kind="stable")                           # by landmark, then time
    ks, lab_s = key[order], lab[order]
    cx, cy = np.cumsum(wx[order]), np.cumsum(wy[order])
    last = np.searchsorted(ks, key, side="right") - 1                # the last beam of (landmark, pose) in the order
    fb = np.searchsorted(lab_s, lab, side="left")                     # the landmark's first beam in the order
    sx = cx[last] - np.where(fb > 0, cx[np.maximum(fb - 1, 0)], 0)
    sy = cy[last] - np.where(fb > 0, cy[np.maximum(fb - 1, 0)], 0)
    sn = last + 1 - fb
    return sx / sn, sy / sn


def test_layout_getter_equals_the_host_formula():
    from icmslam_hip import SweepEngine
    sizes = [16, 17, 1024, 1025, 4096, 16383, 16384, 24000, 33000, 35000, 40001, 48000, 65535, 65536, 70000]
    sc = pb.layout_scene(70000)
    for n in sizes:
        eng = SweepEngine(pb.cfg_of(sc))
        eng.upload(sc.ranges[:, :n], sc.odometry[:, :n], sc.u[:, :n])
        got = eng.entry_layout()
        eng.close()
        want = entry_layout(n)
        print(n, got)
        assert {k: got[k] for k in want} == want
    assert {entry_layout(n)["chunk_poses"] for n in sizes} == {16, 32, 64}


@pytest.mark.parametrize("name", pb.LAYOUT)
def test_targets_against_extended_precision_and_one_sweep_against_the_c_oracle(name):
    sc = pb.scene(name)
    K0 = sc.map.shape[1]
    out = {}
    for path in ("hier", "sort"):
        eng = _engine(sc)
        eng.set_entry_path(path)
        eng.set_debug(True)
        x = sc.x_init.copy()
        mo, co_, K = eng.sweep(sc.map, x, sc.x0, K0, "redblack")
        assert eng.entry_path() == path
        lab, tx, ty = eng.association()
        out[path] = (lab.copy(), tx.copy(), ty.copy(), x, mo[:, :K].copy(), co_.copy(), K, eng.raw_map(), eng.kept_beams())
        eng.close()
    lab, tx, ty, x, m, cnt, K, (yr, cr, la), kept = out["hier"]
    off, bk, d, bx, by = kept
    xo = sc.x_init.copy()
    mc, cntc, Kc, (yrc, crc, lac), labc, offc = _oracle_sweep(sc, xo, sc.map, K0)
    assert np.array_equal(off, offc)
    assert np.array_equal(lab, labc), "labels == the C oracle's"
    rx, ry = _ref_targets(off, bx, by, lab, sc.x_init)
    err = float(max(np.abs(tx - rx).max(), np.abs(ty - ry).max()))
    ls, sx_, sy_ = out["sort"][:3]
    assert np.array_equal(ls, lab)
    dsort = float(max(np.abs(tx - sx_).max(), np.abs(ty - sy_).max()))
    dm, dx = np.abs(m - mc).max() if K == Kc else np.inf, np.abs(x - xo).max()
    draw = np.abs(yr[:, :la] - yrc[:, :lac]).max() if la == lac else np.inf
    lay = entry_layout(sc.T)
    print("%s (CH %d, G %d, nsuper %d): %d beams, max|target - longdouble| %.3e m, max|hier - sort| %.3e, "
          "max|draw| %.2e max|dmap| %.2e max|dx| %.2e"
          % (name, lay["chunk_poses"], lay["chunk_group"], lay["nsuper"], lab.size, err, dsort, draw, dm, dx))
    assert err <= 1e-11
    assert dsort <= 1e-12
    assert la == lac and np.array_equal(cr[:la], crc[:lac]) and draw <= TOL
    assert K == Kc and np.array_equal(cnt, cntc) and dm <= TOL and dx <= TOL


def test_sequential_schedule_against_the_c_oracle():
    sc = pb.scene("layout:1025")
    eng = _engine(sc)
    x = sc.x_init.copy()
    mo, cnt, K = eng.sweep(sc.map, x, sc.x0, sc.map.shape[1], "sequential")
    assert eng.entry_path() == "hier"
    yr, cr, la = eng.raw_map()
    eng.close()
    xo = sc.x_init.copy()
    mc, cntc, Kc, (yrc, crc, lac), _, _ = _oracle_sweep(sc, xo, sc.map, sc.map.shape[1], "sequential")
    assert K == Kc and np.array_equal(cnt, cntc) and np.abs(mo[:, :K] - mc).max() <= TOL
    assert la == lac and np.abs(yr[:, :la] - yrc[:, :lac]).max() <= TOL and np.abs(x - xo).max() <= TOL


class _Like:
    pass


def _dense_ring_scene():
    from test_gpu_edge import _dense_ring_case
    lm, scans, x_true, u, cfgd = _dense_ring_case()
    sc = _Like()
    sc.map, sc.ranges, sc.x_init, sc.x0, sc.u, sc.odometry = lm, scans, x_true.copy(), x_true[:, 0].copy(), u, x_true.copy()
    sc.T, sc.config, sc.label = x_true.shape[1], cfgd, "dense ring"
    return sc


@pytest.mark.parametrize("name", pb.LIMITS + ["dense"])
def test_fallback_rule_is_exact(name):
    sc = _dense_ring_scene() if name == "dense" else pb.scene(name)
    K0 = sc.map.shape[1]
    xo = sc.x_init.copy()
    mc, cntc, Kc, _, labc, offc = _oracle_sweep(sc, xo, sc.map, K0)
    r = pb.reach(sc, offc, labc)
    want = pb.expected_path(r)
    print("%s: entries per pose <= %d, labels per chunk <= %d, per superchunk <= %d -> %s"
          % (sc.label, r["entries"].max(), r["per_chunk"].max(), r["per_super"].max(), want))
    if name == "dense":
        assert want == "sort"
    # the host looks in the middle of the sweep
    eng = _engine(sc)
    x = sc.x_init.copy()
    mo, cnt, K = eng.sweep(sc.map, x, sc.x0, K0, "redblack")
    assert eng.entry_path() == want
    assert K == Kc and np.array_equal(cnt, cntc) and np.abs(mo[:, :K] - mc).max() <= TOL and np.abs(x - xo).max() <= TOL
    eng.close()
    # queued whole: an overflow repeats the sweep with the host looking
    eng = _engine(sc)
    eng.set_state(sc.map, sc.x_init, sc.x0)
    eng.sweep_device("redblack")
    assert eng.entry_path() == want
    x, m, cnt, K = eng.get_state()
    assert K == Kc and np.array_equal(cnt, cntc) and np.abs(m[:, :K] - mc).max() <= TOL and np.abs(x - xo).max() <= TOL
    if want == "sort" and name != "dense":
        # sticky: the next sweep stays on the sort-based pipeline ...
        eng.sweep_device("redblack")
        assert eng.entry_path() == "sort"
        # ... until set_state: a map of the sparse band only (the patch's beams become one fresh label per pose) fits
        eng.set_state(sc.map[:, :sc.n_base], sc.x_init, sc.x0)
        eng.sweep_device("redblack")
        assert eng.entry_path() == "hier"
        x, m, cnt, K = eng.get_state()
        xo = sc.x_init.copy()
        mc, cntc, Kc, _, _, _ = _oracle_sweep(sc, xo, sc.map[:, :sc.n_base], sc.n_base)
        assert K == Kc and np.array_equal(cnt, cntc) and np.abs(m[:, :K] - mc).max() <= TOL and np.abs(x - xo).max() <= TOL
    eng.close()


def test_ranks_of_new_landmarks_in_sweeps_without_the_scan_kernels():
    sc = pb.scene("ranks")
    lay = entry_layout(sc.T)
    eng = _engine(sc)
    assert eng.entry_layout()["nchunks"] == lay["nchunks"] > 512
    eng.set_state(sc.map, sc.x_init, sc.x0)
    xo, mv, la = sc.x_init.copy(), sc.map, sc.map.shape[1]
    for it in range(3):
        K_in = la
        eng.sweep_device("redblack")
        info = eng.entry_layout()
        assert eng.entry_path() == "hier"
        assert info["scan_ran"] == (it == 0), "sweeps 2 and 3 run without the scan kernels"
        x, m, cnt, K = eng.get_state()
        mv, cntc, la, _, labc, offc = _oracle_sweep(sc, xo, mv, la)
        r = pb.reach(sc, offc, labc) if it == 0 else None
        pose = np.repeat(np.arange(sc.T), np.diff(offc))
        # the poses that create a landmark this sweep: labels beyond the map the sweep started from
        creators = np.unique(pose[labc >= K_in])
        cchunks = np.unique(creators // lay["chunk_poses"])
        print("sweep %d: scan kernels %s, creating poses %d in chunks %s, K %d/%d, max|dmap| %.2e max|dx| %.2e"
              % (it + 1, info["scan_ran"], creators.size, cchunks.tolist(), K, la,
                 np.abs(m[:, :K] - mv).max() if K == la else np.inf, np.abs(x - xo).max()))
        assert 0 in cchunks and lay["nchunks"] - 1 in cchunks and (cchunks > 512).sum() >= 4
        assert K == la and np.array_equal(cnt, cntc)
        for j in range(K):   # column by column: a wrong rank permutes them
            assert np.abs(m[:, j] - mv[:, j]).max() <= TOL, "map column %d" % j
        assert np.abs(x - xo).max() <= TOL
        if r is not None:
            assert set(r["creators"].tolist()) == set(creators.tolist())
    eng.close()


@pytest.mark.parametrize("T,world,ch_all,ch_rank", [(70000, 2, 64, 32), (48000, 3, 32, 16)])
def test_virtual_ranks_with_a_different_chunking(T, world, ch_all, ch_rank):
    import torch
    from icmslam_hip import SweepEngine
    from icmslam_hip.sharded import NoComm, ShardedSweep, partition, run_virtual_ranks
    sc = pb.layout_scene(T, clutter=[3, T // 2 + 5, T - 7], label="shards %d" % T)
    eng = _engine(sc)
    assert eng.entry_layout()["chunk_poses"] == ch_all
    eng.set_state(sc.map, sc.x_init, sc.x0)
    sweeps = 2
    for _ in range(sweeps):
        eng.sweep_device("redblack")
    assert eng.entry_path() == "hier"
    x1, m1, c1, K1 = eng.get_state()
    eng.close()
    blk, parts = partition(sc.T, world)
    engines, runners, stats = [], [], None
    for r, (a, b) in enumerate(parts):
        e = SweepEngine(pb.cfg_of(sc))
        e.upload(sc.ranges, sc.odometry, sc.u, t_begin=a, t_end=b)
        assert e.entry_layout()["chunk_poses"] == ch_rank
        run = ShardedSweep(e, r, world, sc.T, comm=NoComm(), stats=stats)
        stats = run.stats
        run.set_state(sc.map, sc.x_init, sc.x0)
        engines.append(e)
        runners.append(run)
    run_virtual_ranks(runners, sweeps)
    torch.cuda.synchronize()
    for e in engines:
        x, m, c, K = e.get_state()
        d = np.abs(x - x1).max()
        print("T %d on %d ranks: K %d/%d max|dx| %.2e" % (T, world, K, K1, d))
        assert K == K1 and np.array_equal(c, c1) and np.abs(m[:, :K] - m1[:, :K1]).max() <= TOL and d <= TOL
    for e in engines:
        e.close()
