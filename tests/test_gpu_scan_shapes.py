"""The per-scan kernels on wide scans (tests/scan_shapes.py): full-length runs (k = 64), more than 64 and more than 128
runs, kept beams and entries per scan, the 256-slot relaunch with multi-beam runs, scans without beams between wide
ones, B = 64, 65, 1440 and ICM_MAX_BEAMS -- against the oracles: kept beams and runs bit for bit and beam for beam,
labels and counters exact, real values <= 1e-9.

k_prefilter / k_run_build   kept beams == oracle.prefilter_all, runs == oracle.cut_runs (cut after kRunCap beams too)
k_assoc_runs                run form == beam form == brute force, beam by beam; its count of unsettled runs ==
                            oracle.run_decision's (the batch loop over runs 64.., its reload of sum / count / offset)
whole sweeps                2 sweeps, red-black and sequential, both entry pipelines, against the C oracle
k_init_pass                 the causal pass over scans of ~360 kept beams against the C oracle
energy forms                per-beam and per-entry (beyond 64 entries: the out-of-register path) against the C oracle
shards                      2 and 3 virtual ranks, ghost scans of 180 multi-beam runs (k_assoc_runs<false, 256>, on
                            the solve stream while Mapa.filtrar rebuilds the search grid on the side stream)
the beam limit              B = ICM_MAX_BEAMS + 1 refused at upload; the handle then takes a legal sequence
"""
import os
import re

import numpy as np
import pytest

import scan_shapes as ss
from oracle import icm_oracle as o
from util import ROOT, check_runs

pytestmark = pytest.mark.gpu

TOL = 1e-9
RINGS = [("ring", 64), ("ring", 65), ("ring", 1440), ("ring", 1462)]


def _max_beams():
    h = open(os.path.join(ROOT, "include", "icmslam.h")).read()
    return int(re.search(r"#define ICM_MAX_BEAMS (\d+)", h).group(1))


def _engine(sc):
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    cfg = ConfigICM(D=sc.config)
    eng = SweepEngine(cfg)
    eng.upload(sc.ranges, sc.odometry, sc.u)
    return eng, cfg


def _reached(sc):
    r = sc.reach
    over = [sum(max(n - 64 * b, 0) for n in r["runs"]) for b in (1, 2)]
    return ("%s B=%d: capped runs %d, most runs per pose %d, runs past index 64 / 128: %d / %d, unsettled runs past index "
            "64 / 128: %d / %d, labels (entries) per pose <= %d, most kept beams per pose %d"
            % (sc.kind, sc.B, r["capped"], max(r["runs"]), over[0], over[1], r["unsettled_batch"][1] + r["unsettled_batch"][2],
               r["unsettled_batch"][2], max(r["labels"]), max(r["kept"])))


@pytest.mark.parametrize("kind,B", RINGS + [("dense", 1440), ("trunks", 1440)])
def test_kept_beams_and_runs_equal_the_oracle(kind, B):
    from oracle import c_oracle as co
    sc = ss.scene(kind, B)
    assert B <= _max_beams()
    eng, cfg = _engine(sc)
    off, bk, d, bx, by = eng.kept_beams()
    kept = o.prefilter_all(sc.ranges, ss.oracle_config(sc))
    keptc = co.prefilter(cfg, sc.ranges)
    assert np.array_equal(off, keptc[0]) and np.array_equal(bk, keptc[1])
    rows = np.concatenate([kz for kz in kept if kz.ndim == 2 and kz.shape[0]])
    assert np.array_equal(d, rows[:, 0]) and np.array_equal(bx, rows[:, 2]) and np.array_equal(by, rows[:, 3]), "bit for bit"
    check_runs(eng, sc.thr)
    roff, c, sb, r, k, f = eng.runs()
    for t in range(sc.T):
        body = np.stack((bx[off[t]:off[t + 1]], by[off[t]:off[t + 1]]), axis=1)
        mine = [(int(f[q]), int(k[q])) for q in range(roff[t], roff[t + 1])]
        assert mine == o.cut_runs(body, sc.thr), "runs of scan %d" % t
    print(_reached(sc), "| device: %d runs, %d of 64 beams" % (len(k), int((k == 64).sum())))
    assert int((k == 64).sum()) == sc.reach["capped"]
    eng.close()


def _phase_a(eng, sc, form, brute=False):
    eng.set_assoc_form(form)
    eng.set_brute_force(brute)
    eng.set_debug(True)
    eng.set_entry_path("hier")
    eng.set_state(sc.map, sc.x_init, sc.x0)
    before = eng.run_counts()[1]
    eng.sweep_device("sequential")
    bbb = eng.run_counts()[1] - before
    out = (eng.association()[0].copy(), eng.raw_map(), eng.get_state(), bbb, eng.last_stats())
    eng.set_brute_force(False)
    eng.set_debug(False)
    return out


@pytest.mark.parametrize("kind,B", [("ring", 1440), ("ring", 1462), ("dense", 1440), ("ring", 65)])
def test_phase_a_run_form_equals_beam_form_and_brute_force(kind, B):
    """Sweep 1, sequential, from the scene's map: the label of every kept beam from k_assoc_runs equals the beam-by-beam
    kernel's, the brute-force kernel's and the C oracle's; counters and K exact, raw map, map and poses <= 1e-9.  In the
    ring scene (<= 96 labels: no relaunch) the device's count of runs that went beam by beam equals the number of runs
    oracle.run_decision does not settle (no run lies within 1e-5 dist_thr of a margin of the test)."""
    from oracle import c_oracle as co
    sc = ss.scene(kind, B)
    eng, cfg = _engine(sc)
    res = {f: _phase_a(eng, sc, *f) for f in (("runs",), ("beams",), ("beams", True))}
    eng.close()
    runs, beams, brute = res[("runs",)], res[("beams",)], res[("beams", True)]
    a = {}
    xc = sc.x_init.copy()
    mc, cntc, Kc, (yr, cr, lr) = co.sweep(cfg, co.prefilter(cfg, sc.ranges), sc.u, sc.odometry, sc.x0, sc.map, xc,
                                          sc.map.shape[1], "sequential", assoc=a)
    for name, other in (("beam form", beams), ("brute force", brute)):
        assert np.array_equal(runs[0], other[0]), "labels differ from the %s on %d beams" % (name, int((runs[0] != other[0]).sum()))
        (ya, ca, la), (yb, cb, lb) = runs[1], other[1]
        assert la == lb and np.array_equal(ca, cb) and np.abs(ya - yb).max() <= TOL
        assert runs[2][3] == other[2][3] and np.array_equal(runs[2][2], other[2][2])
        assert np.abs(runs[2][0] - other[2][0]).max() <= TOL and np.abs(runs[2][1] - other[2][1]).max() <= TOL
    assert np.array_equal(runs[0], a["labels"]), "labels differ from the C oracle's on %d beams" % int((runs[0] != a["labels"]).sum())
    (y, cnt, lact), (x, m, c, K) = runs[1], runs[2]
    assert lact == lr and np.array_equal(cnt, cr) and np.abs(y[:, :lact] - yr[:, :lact]).max() <= TOL
    assert K == Kc and np.array_equal(c, cntc) and np.abs(m[:, :K] - mc).max() <= TOL and np.abs(x - xc).max() <= TOL
    print(_reached(sc), "| labels exact (%d beams); beam by beam: device %d, oracle %d; entries %d"
          % (runs[0].size, runs[3], sc.reach["unsettled"], runs[4]["entries"]))
    if max(sc.reach["labels"]) <= 96:
        assert sc.reach["min_margin"] > ss.MARGIN_TOL * sc.thr
        assert runs[3] == sc.reach["unsettled"], "runs that went beam by beam"


def _sweeps_against_c_oracle(sc, schedule, path=None, energy=None, sweeps=2):
    from oracle import c_oracle as co
    eng, cfg = _engine(sc)
    if path:
        eng.set_entry_path(path)
    if energy:
        eng.set_energy_form(energy)
    eng.set_state(sc.map, sc.x_init, sc.x0)
    keptc = co.prefilter(cfg, sc.ranges)
    xc = sc.x_init.copy()
    mvc, lac = sc.map, sc.map.shape[1]
    for it in range(sweeps):
        eng.sweep_device(schedule)
        x, m, cnt, K = eng.get_state()
        stats = eng.last_stats()
        mvc, cntc, lac, raw = co.sweep(cfg, keptc, sc.u, sc.odometry, sc.x0, mvc, xc, lac, schedule)
        dm, dx = np.abs(m[:, :K] - mvc).max() if K == lac else np.inf, np.abs(x - xc).max()
        print("%s B=%d %s %s %s sweep %d: K %d/%d, %d entries, max|dmap| %.2e max|dx| %.2e"
              % (sc.kind, sc.B, schedule, path or "", energy or "", it + 1, K, lac, stats["entries"], dm, dx))
        assert K == lac and np.array_equal(cnt, cntc) and dm <= TOL and dx <= TOL
    eng.close()


@pytest.mark.parametrize("path", ["hier", "sort"])
@pytest.mark.parametrize("schedule", ["redblack", "sequential"])
@pytest.mark.parametrize("kind,B", RINGS + [("dense", 1440)])
def test_two_sweeps_against_the_c_oracle(kind, B, schedule, path):
    _sweeps_against_c_oracle(ss.scene(kind, B), schedule, path)


@pytest.mark.parametrize("form", ["beam", "entry"])
@pytest.mark.parametrize("kind", ["ring", "dense"])
def test_energy_forms_against_the_c_oracle(kind, form):
    """The cross-check energies over more than 64 kept beams per pose (per-beam form) and more than 64 entries per pose
    (per-entry form past its in-register case)."""
    sc = ss.scene(kind, 1440)
    assert max(sc.reach["kept"]) > 64 and max(sc.reach["labels"]) > 64
    print(_reached(sc))
    _sweeps_against_c_oracle(sc, "redblack", energy=form)


def test_init_pass_against_the_c_oracle():
    from oracle import c_oracle as co
    sc = ss.scene("trunks", 1440)
    eng, cfg = _engine(sc)
    x0 = sc.odometry[:, 0].copy()
    x, y, cnt, lact, c0 = eng.init_pass(x0)
    eng.close()
    ocfg = ss.oracle_config(sc)
    kept = o.prefilter_all(sc.ranges, ocfg)
    st = o.MapState(ocfg)
    y0, c0n = o.cluster_first_scan(st, np.zeros((2, ocfg.L)), o.project_beams(x0, kept[0][:, 2:4]))
    assert np.array_equal(c0, c0n), "clusters of the first scan"
    xc, yc, cc, lc = co.init_pass(cfg, co.prefilter(cfg, sc.ranges), sc.u, sc.odometry, y0, st.cant_obs_i, st.landmarks_actuales)
    n = np.array(sc.reach["kept"])
    dx, dy = np.abs(x - xc).max(), np.abs(y - yc).max()
    print("trunks init pass: kept beams per scan up to %d, %d scans with more than 64, %d with more than 128, %d without; "
          "%d labels; max|dx| %.2e max|dy| %.2e" % (n.max(), int((n > 64).sum()), int((n > 128).sum()), int((n == 0).sum()), lact, dx, dy))
    assert lact == lc and np.array_equal(cnt, cc) and dy <= TOL and dx <= TOL


@pytest.mark.parametrize("world", [2, 3])
def test_virtual_ranks_match_unsharded_on_wide_scans(world):
    """Two sweeps sharded == unsharded: K, counters exact, map and every pose <= 1e-9.  A ghost scan this wide keeps the
    ghost pose's association running well past k_rec_push, so Mapa.filtrar -- which rewrites the search grid that
    association reads -- must be ordered behind it (queue_filtrar waits for ev_gh1): without that, the first pose of each
    shard was solved against a ghost pose associated on a half-rebuilt grid (7e-3 off after one sweep)."""
    import torch
    from icmslam_hip.sharded import NoComm, ShardedSweep, partition, run_virtual_ranks
    sc = ss.scene("ring", 1440)
    eng, cfg = _engine(sc)
    eng.set_state(sc.map, sc.x_init, sc.x0)
    sweeps = 2
    for _ in range(sweeps):
        eng.sweep_device("redblack")
    x1, m1, c1, K1 = eng.get_state()
    eng.close()
    blk, parts = partition(sc.T, world)
    ghosts = [a - 1 for a, _ in parts[1:]]
    assert all(sc.reach["multi_beam_runs"][g] > 64 for g in ghosts), "ghost scans of more than 64 multi-beam runs"
    from icmslam_hip import SweepEngine
    engines, runners, stats = [], [], None
    for r, (a, b) in enumerate(parts):
        e = SweepEngine(cfg)
        e.upload(sc.ranges, sc.odometry, sc.u, t_begin=a, t_end=b)
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
        print("world %d, ghost poses %s (%s runs): K %d/%d max|dx| %.2e" % (world, ghosts, [sc.reach["runs"][g] for g in ghosts], K, K1, d))
        assert K == K1 and np.array_equal(c, c1) and np.abs(m[:, :K] - m1[:, :K1]).max() <= TOL and d <= TOL
    for e in engines:
        e.close()


def test_upload_refuses_more_beams_than_the_limit_and_the_handle_stays_usable():
    from icmslam_hip import _lib
    limit = _max_beams()
    assert limit == 160 * 1024 // (4 * 28)
    sc = ss.scene("ring", 65)
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    eng = SweepEngine(ConfigICM(D=sc.config))
    wide = np.full((limit + 1, sc.T), ss.RING_R)
    with pytest.raises(NotImplementedError, match="ICM_MAX_BEAMS = %d" % limit):
        eng.upload(wide, sc.odometry, sc.u)
    assert eng.last_rc == _lib.ICM_ERR_UNSUPPORTED
    eng.upload(sc.ranges, sc.odometry, sc.u)     # the same handle, a legal sequence
    from oracle import c_oracle as co
    cfg = eng.config
    eng.set_state(sc.map, sc.x_init, sc.x0)
    eng.sweep_device("redblack")
    x, m, cnt, K = eng.get_state()
    eng.close()
    xc = sc.x_init.copy()
    mc, cntc, Kc, _ = co.sweep(cfg, co.prefilter(cfg, sc.ranges), sc.u, sc.odometry, sc.x0, sc.map, xc, sc.map.shape[1], "redblack")
    print("B = %d refused; B = %d afterwards on the same handle: K %d/%d max|dx| %.2e" % (limit + 1, sc.B, K, Kc, np.abs(x - xc).max()))
    assert K == Kc and np.array_equal(cnt, cntc) and np.abs(m[:, :K] - mc).max() <= TOL and np.abs(x - xc).max() <= TOL
