"""Edge cases and size-independent properties of the HIP sweep."""
import os

import numpy as np
import pytest

from util import Cfg, ROOT, dataset, gold

pytestmark = pytest.mark.gpu


def _oracle_redblack(cfg, zz, odo, u, x_init, map_init, lact, T):
    from oracle import icm_oracle as o
    ocfg = o.OracleConfig.from_config(cfg)
    st = o.MapState(ocfg, lact)
    x = np.ascontiguousarray(x_init[:, :T]).copy()
    m, x = o.sweep(ocfg, st, zz[:, :T], u[:, :T], odo[:, :T], odo[:, 0], map_init.copy(), x, schedule="redblack")
    return m, x, st


@pytest.mark.parametrize("form", ["moments", "beam", "entry"])
def test_anisotropic_weights_match_oracle(form):
    """Q, R not multiples of the identity and cte_odom != 1: exercises the theta-dependent
    scatter term of the grouped energy forms and every weight of the priors."""
    from icmslam_hip import SweepEngine
    zz, odo, u = dataset()
    init = gold("init_pass.npz")
    T = 300
    cfg = Cfg(cota=20.0, Q=np.diag([2.0, 0.5]), R=np.diag([1.5, 0.7, 2.0]), cte_odom=0.3)
    eng = SweepEngine(cfg)
    eng.upload(zz[:, :T], odo[:, :T], u[:, :T])
    eng.set_energy_form(form)
    x = np.ascontiguousarray(init["x_init"][:, :T]).copy()
    mo, co, K = eng.sweep(init["map_init"], x, odo[:, 0], int(init["landmarks_actuales"]), "redblack")
    eng.close()
    mref, xref, st = _oracle_redblack(cfg, zz, odo, u, init["x_init"], init["map_init"], int(init["landmarks_actuales"]), T)
    d = np.abs(x - xref).max(axis=0)
    print("anisotropic (%s): max|dx| %.3e, poses above 1e-9: %d" % (form, d.max(), int((d > 1e-9).sum())))
    assert K == mref.shape[1] and np.abs(mo[:, :K] - mref).max() <= 1e-9
    assert d.max() <= 1e-9


def test_first_scan_without_beams_returns_inputs():
    """reference scripts/ICM_ROS.py:133-135."""
    from icmslam_hip import SweepEngine
    zz, odo, u = dataset()
    init = gold("init_pass.npz")
    T = 60
    z2 = zz[:, :T].copy()
    z2[:, 0] = 10.0  # nothing in range in scan 0
    eng = SweepEngine(Cfg(cota=5.0))
    eng.upload(z2, odo[:, :T], u[:, :T])
    x = np.ascontiguousarray(init["x_init"][:, :T]).copy()
    x_before = x.copy()
    assert eng.sweep(init["map_init"], x, odo[:, 0], 11, "sequential") is None
    assert np.array_equal(x, x_before)
    eng.close()


def test_last_pose_without_beams_raises_index_error():
    """reference scripts/ICM_ROS.py:144 indexes x[:, T]."""
    from icmslam_hip import SweepEngine
    zz, odo, u = dataset()
    init = gold("init_pass.npz")
    T = 60
    z2 = zz[:, :T].copy()
    z2[:, -1] = 10.0
    eng = SweepEngine(Cfg(cota=5.0))
    eng.upload(z2, odo[:, :T], u[:, :T])
    x = np.ascontiguousarray(init["x_init"][:, :T]).copy()
    for sch in ("sequential", "redblack"):
        with pytest.raises(IndexError):
            eng.sweep(init["map_init"], x, odo[:, 0], 11, sch)
    eng.close()


def test_single_beam_scans_and_ragged_counts():
    """Scans with 0, 2, few and many kept beams in one sequence; the pre-filter's '<= 1 beam
    in range -> empty' rule (scripts/ICM_SLAM_tools.py:41,55)."""
    from icmslam_hip import SweepEngine
    from oracle import icm_oracle as o
    zz, odo, u = dataset()
    T = 40
    z2 = zz[:, :T].copy()
    z2[:, 5] = 10.0
    z2[:, 6] = 10.0
    z2[90, 6] = 3.0          # one beam only (median filter removes it anyway)
    z2[:, 7] = 10.0
    z2[60:63, 7] = 4.0       # three adjacent beams -> median keeps some
    eng = SweepEngine(Cfg())
    eng.upload(z2, odo[:, :T], u[:, :T])
    off, bk, d, bx, by = eng.kept_beams()
    eng.close()
    kept = o.prefilter_all(z2, o.OracleConfig())
    for t in range(T):
        ref = kept[t] if kept[t].ndim == 2 else np.zeros((0, 4))
        assert off[t + 1] - off[t] == ref.shape[0]
        assert np.array_equal(d[off[t]:off[t + 1]], ref[:, 0]) and np.array_equal(bx[off[t]:off[t + 1]], ref[:, 2])
    assert off[6] == off[5] and off[7] == off[6]


def test_brute_force_equals_grid_at_s1_size():
    """Association labels of the grid search vs the literal all-landmarks search on the S1
    workload (10k poses, 1k landmarks): identical labels, hence identical sweeps."""
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.synthetic import WORKLOADS, make_workload
    wl = make_workload(*WORKLOADS["S1"])
    eng = SweepEngine(ConfigICM(D=wl.config))
    eng.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
    eng.set_debug(True)
    out = []
    for brute, form in ((False, "beams"), (True, "beams"), (False, "runs")):
        eng.set_brute_force(brute)
        eng.set_assoc_form(form)
        eng.set_state(wl.map_init, wl.x_init, wl.x0)
        eng.sweep_device("redblack")
        out.append((eng.association()[0].copy(),) + eng.get_state())
    eng.close()
    # beam by beam, grid search against the all-landmarks search: the same labels, and then the same arithmetic
    assert np.array_equal(out[0][0], out[1][0])
    for a, b in zip(out[0][1:], out[1][1:]):
        assert np.array_equal(a, b)
    assert (out[0][0] >= 0).all()
    # by runs (the default form): the same labels and counters; the per-entry sums are added up run by run, so real-valued
    # state agrees to rounding (<= 1e-9 like everywhere; bit-identical poses are reported, not required)
    assert np.array_equal(out[2][0], out[1][0])
    x2, m2, c2, K2 = out[2][1:]
    x1, m1, c1, K1 = out[1][1:]
    assert K2 == K1 and np.array_equal(c2, c1)
    print("run form vs brute force: max|dmap| %.2e  max|dx| %.2e  poses bit-identical: %s" % (np.abs(m2 - m1).max(), np.abs(x2 - x1).max(), np.array_equal(x2, x1)))
    assert np.abs(m2 - m1).max() <= 1e-9 and np.abs(x2 - x1).max() <= 1e-9


def test_prefilter_edge_cases_match_the_oracle():
    """filtrar_z on hand-made scans against the NumPy oracle (scripts/ICM_SLAM_tools.py:22-58), row for row: nothing in
    range, one beam in range, isolated beams only, neighbours that sit more than eight places apart in the list of
    in-range beams (only the all-beams step can find them), exactly coincident points (distance zero counts as 100),
    runs that end at the 64- and 128-beam boundaries of the kernel's chunks, and a threshold of 100 and more (every
    in-range beam stays)."""
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.synthetic import make_workload
    from oracle import icm_oracle as oc
    wl = make_workload(300, 49, 360)
    B, rmax = 360, float(wl.config["rango_laser_max"])
    rng = np.random.default_rng(11)
    far = rmax + 1.0
    scans = []
    scans.append(np.full(B, far))                                   # nothing in range
    z = np.full(B, far); z[100:103] = 4.0; scans.append(z)          # median-3 leaves one beam in range
    z = np.full(B, far); z[10:13] = 3.0; z[200:203] = 3.0; scans.append(z)   # two lone beams, 3+ m apart
    z = np.full(B, far)                                             # partners 180 degrees apart at 0.3 m: 0.6 m between them,
    for k in range(0, 170, 9):                                      # with unrelated in-range beams in between in the list
        z[k:k + 3] = 0.3; z[k + 180:k + 183] = 0.3
    z[90:93] = 9.0
    scans.append(z)
    z = np.full(B, far); z[0:3] = 0.0; z[120:123] = 0.0; z[240:243] = 0.0; scans.append(z)   # coincident points at the origin
    for n in (63, 64, 65, 127, 128, 129):                           # a wall of n in-range beams
        z = np.full(B, far); z[5:5 + n] = 5.0 + 0.01 * rng.random(n); scans.append(z)
    for _ in range(20):                                             # random clutter
        z = np.where(rng.random(B) < 0.25, rng.uniform(0.2, rmax, B), far); scans.append(z)
    S = np.ascontiguousarray(np.array(scans))                       # (n, B) pose-major
    T = S.shape[0]
    for thr in (float(wl.config["dist_thr"]), 0.05, 100.0, 250.0):
        cfgd = dict(wl.config); cfgd["dist_thr"] = thr
        cfg = ConfigICM(D=cfgd)
        eng = SweepEngine(cfg)
        eng.upload(S, np.zeros((3, T)), np.zeros((2, T)), pose_major=True)
        off, bk, d, bx, by = eng.kept_beams()
        eng.close()
        ocfg = oc.OracleConfig.from_config(cfg)
        for t in range(T):
            rows = oc.filtrar_z(S[t], ocfg)
            a, b = int(off[t]), int(off[t + 1])
            assert b - a == len(rows), (thr, t, b - a, len(rows))
            if len(rows):
                assert np.array_equal(d[a:b], rows[:, 0]) and np.array_equal(bk[a:b] * np.pi / 180.0, rows[:, 1])
                assert np.array_equal(bx[a:b], rows[:, 2]) and np.array_equal(by[a:b], rows[:, 3])


def test_crowded_neighbourhoods_take_the_rest_of_the_record_and_the_walk():
    """The cell records of the grid search hold the first two candidates where every beam reads them and the other two
    where only the lanes that need them do (and more than four send the beam down the range walk): a reference map with
    decoys 0.25 .. 0.9 m around every landmark -- neighbourhoods of 1 .. 12 candidates, exact mirror images for ties --
    must give the labels of the literal all-landmarks search, beam for beam."""
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.synthetic import make_workload
    wl = make_workload(1350, 400, 360)   # (one lane through a 50 m field, ends inside it)
    rng = np.random.default_rng(5)
    m0 = wl.map_init
    parts = [m0]
    for k, r in enumerate((0.25, 0.45, 0.7, 0.9)):
        ang = rng.uniform(0, 2 * np.pi, m0.shape[1])
        keep = rng.random(m0.shape[1]) < (0.7, 0.5, 0.4, 0.3)[k]
        d = r * np.stack((np.cos(ang), np.sin(ang)))
        parts.append((m0 + d)[:, keep])
        if k == 1:   # mirror images: two candidates at exactly the same distance from points on the landmark's bearing
            parts.append((m0 - d)[:, keep])
    m = np.ascontiguousarray(np.concatenate(parts, axis=1))
    assert m.shape[1] > 3 * m0.shape[1]
    cfgd = dict(wl.config)
    cfgd["L"] = m.shape[1] + 4096
    eng = SweepEngine(ConfigICM(D=cfgd))
    eng.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
    eng.set_debug(True)
    out = []
    for brute, form in ((False, "beams"), (True, "beams"), (False, "runs")):
        eng.set_brute_force(brute)
        eng.set_assoc_form(form)
        eng.set_state(m, wl.x_init, wl.x0)
        eng.sweep_device("redblack")
        out.append((eng.association()[0].copy(),) + eng.get_state())
    n_runs, beam_by_beam = eng.run_counts()
    eng.close()
    assert np.array_equal(out[0][0], out[1][0])
    for a, b in zip(out[0][1:], out[1][1:]):
        assert np.array_equal(a, b)
    # the decoys are really in play: a share of the beams goes to them (10 % here)
    assert (out[0][0] >= m0.shape[1]).mean() > 0.05
    # the run form on the same crowded map (few runs are settled by their bounding circle here): same labels, same
    # counters, state to rounding
    assert np.array_equal(out[2][0], out[1][0])
    assert out[2][4] == out[1][4] and np.array_equal(out[2][3], out[1][3])
    print("crowded map, run form: %d of %d runs beam by beam; vs brute force max|dmap| %.2e max|dx| %.2e"
          % (beam_by_beam, n_runs, np.abs(out[2][2] - out[1][2]).max(), np.abs(out[2][1] - out[1][1]).max()))
    assert beam_by_beam > n_runs // 2
    assert np.abs(out[2][2] - out[1][2]).max() <= 1e-9 and np.abs(out[2][1] - out[1][1]).max() <= 1e-9


def test_s2_full_size_properties():
    """BASELINE configs[3] at full size (100k poses / 10k landmarks / 720 beams): the sweep is
    deterministic (two runs bit-equal), the sharded phase path equals the unsharded one, every
    kept beam gets a label below landmarks_actuales, the counters sum to the kept beams, and
    the map change between sweeps (calc_cambio) shrinks."""
    import torch
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.sharded import NoComm, ShardedSweep, partition, run_virtual_ranks
    from icmslam_hip.synthetic import WORKLOADS, make_workload
    wl = make_workload(*WORKLOADS["S2"])
    cfg = ConfigICM(D=wl.config)
    eng = SweepEngine(cfg)
    eng.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
    runs, cambio = [], []
    for rep in range(2):
        eng.set_state(wl.map_init, wl.x_init, wl.x0)
        prev = wl.map_init
        for _ in range(5):
            eng.sweep_device("redblack")
            if rep == 0:  # the reference's convergence metric (calc_cambio, scripts/ICM_SLAM_tools.py:490-495)
                _, mm, _, kk = eng.get_state()
                cur = mm[:, :kk]
                dd = np.sqrt(((cur[:, :, None] - prev[:, None, :]) ** 2).sum(axis=0)).min(axis=1)
                cambio.append(float(dd.mean()))
                prev = cur.copy()
        runs.append(eng.get_state())
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)
    x, m, c, K = runs[0]
    yr, cr, la = eng.raw_map()
    st = eng.last_stats()
    assert cr[:la].sum() == st["kept_beams"] == eng.nnz
    eng.set_debug(True)
    eng.sweep_device("redblack")
    lab = eng.association()[0]
    assert lab.min() >= 0 and lab.max() < eng.raw_map()[2]
    eng.close()
    print("S2 mean landmark change per sweep:", ["%.2e" % v for v in cambio], "landmarks", K)
    assert cambio[-1] < 0.5 * cambio[0]
    # sharded (2 virtual ranks, shared statistics buffer) == unsharded, 2 sweeps
    world = 2
    _, parts = partition(wl.T, world)
    engines, runners, stats = [], [], None
    for r, (a, b) in enumerate(parts):
        e = SweepEngine(cfg)
        e.upload(wl.scans[a:b], wl.odometry, wl.u, t_begin=a, t_end=b, pose_major=True, ghost_scan=wl.scans[a - 1] if a else None)
        run = ShardedSweep(e, r, world, wl.T, comm=NoComm(), stats=stats)
        stats = run.stats
        run.set_state(wl.map_init, wl.x_init, wl.x0)
        engines.append(e)
        runners.append(run)
    run_virtual_ranks(runners, 2)
    torch.cuda.synchronize()
    xs, ms, cs, Ks = engines[0].get_state()
    for e in engines:
        e.close()
    e1 = SweepEngine(cfg)
    e1.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
    e1.set_state(wl.map_init, wl.x_init, wl.x0)
    for _ in range(2):
        e1.sweep_device("redblack")
    x1, m1, c1, K1 = e1.get_state()
    e1.close()
    assert Ks == K1 and np.abs(ms - m1).max() <= 1e-9 and np.array_equal(cs, c1)
    d = np.abs(xs - x1).max(axis=0)
    print("S2 sharded x2 vs unsharded: max|dx| %.3e, poses above 1e-9: %d" % (d.max(), int((d > 1e-9).sum())))
    assert d.max() <= 1e-9


def test_landmark_merge_path_matches_oracle():
    """Two map landmarks 0.4 m apart (< dist_thr) split the beams of one trunk; Mapa.filtrar must
    merge them (count-weighted mean, label propagation, renumbering) -- on the GPU (k_fl_components
    .. k_fl_gather), without the host routine; result vs the oracle."""
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.synthetic import make_workload
    from oracle import icm_oracle as o
    wl = make_workload(500, 49, 180)
    cfg = ConfigICM(D=dict(wl.config, cota=3.0))
    # duplicate the three landmarks nearest to the start of the path, shifted by 0.4 m
    d0 = np.hypot(*(wl.map_init - wl.x_true[:2, [0]]))
    near = np.argsort(d0)[:3]
    extra = wl.map_init[:, near] + np.array([[0.4], [0.0]])
    map0 = np.concatenate((wl.map_init, extra), axis=1)
    eng = SweepEngine(cfg)
    eng.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
    x = wl.x_init.copy()
    mo, co, K = eng.sweep(map0, x, wl.x0, map0.shape[1], "redblack")
    yr, cr, la = eng.raw_map()
    Kf, path, pairs = eng.last_filtrar_info()
    eng.close()
    assert path == 1 and pairs >= 6 and Kf == K     # merged on the device, no host routine
    ocfg = o.OracleConfig.from_config(cfg)
    st = o.MapState(ocfg, map0.shape[1])
    xo = wl.x_init.copy()
    mref, xo = o.sweep(ocfg, st, wl.scans.T, wl.u, wl.odometry, wl.x0, map0.copy(), xo, schedule="redblack")
    # the duplicates really were in play and really were merged away
    assert (cr[49:52] > 0).all() and K == mref.shape[1] and K < (cr[:la] >= 3.0).sum()
    assert np.abs(mo[:, :K] - mref).max() <= 1e-9 and np.array_equal(co, st.cant_obs_i)
    assert np.abs(x - xo).max() <= 1e-9


def test_s1_full_size_against_c_oracle():
    """BASELINE configs[2] workload at full size (10 000 poses / 1 000 landmarks / 360 beams), two
    red-black sweeps: HIP vs the compiled C oracle (brute-force association, per-beam energy,
    running-mean recurrence -- the reference's literal arithmetic)."""
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.synthetic import WORKLOADS, make_workload
    from oracle import c_oracle as co
    wl = make_workload(*WORKLOADS["S1"])
    cfg = ConfigICM(D=wl.config)
    eng = SweepEngine(cfg)
    eng.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
    off, bk, d, bx, by = eng.kept_beams()
    keptc = co.prefilter(cfg, wl.scans.T)
    assert np.array_equal(off, keptc[0]) and np.array_equal(bk, keptc[1]) and np.array_equal(bx, keptc[4])
    x = wl.x_init.copy()
    xc = wl.x_init.copy()
    mv, la = wl.map_init, wl.K
    mvc, lac = wl.map_init, wl.K
    for it in range(2):
        mo, cnt, K = eng.sweep(mv, x, wl.x0, la, "redblack")
        mv, la = mo[:, :K].copy(), K
        mvc, cntc, lac, raw = co.sweep(cfg, keptc, wl.u, wl.odometry, wl.x0, mvc, xc, lac, "redblack")
        d_x = np.abs(x - xc).max(axis=0)
        print("S1 sweep %d: K %d/%d  max|dmap| %.2e  max|dx| %.2e  poses above 1e-9: %d" % (it + 1, K, lac, np.abs(mv - mvc).max(), d_x.max(), int((d_x > 1e-9).sum())))
        assert K == lac and np.array_equal(cnt, cntc) and np.abs(mv - mvc).max() <= 1e-9
        assert d_x.max() <= 1e-9
    eng.close()


def _dense_ring_case(grid=0.13, beams=360):
    """360 beams sweeping a ring of landmarks on a 0.13 m grid at ~3 m: neighbouring beams are
    ~0.05 m apart (so the isolated-beam filter keeps them) and hit a new landmark every couple
    of beams -> far more than 96 distinct landmarks in one scan.  `beams` < 360: only the first
    `beams` rows see the ring (the rest read the maximum range and are dropped)."""
    B, T = 360, 6
    g = np.arange(-int(round(3.9 / grid)), int(round(3.9 / grid)) + 1) * grid
    gx, gy = np.meshgrid(g, g)
    lm = np.stack((gx.ravel(), gy.ravel()))
    rr = np.hypot(lm[0], lm[1])
    lm = lm[:, (rr > 2.6) & (rr < 3.4)]
    ang = np.arange(B) * np.pi / 180.0
    x_true = np.zeros((3, T))
    x_true[2] = np.pi / 2
    x_true[0] = 0.002 * np.arange(T)
    scans = np.full((B, T), 10.0)
    for t in range(T):
        a = ang + x_true[2, t] - np.pi / 2
        p = x_true[:2, [t]] + 3.0 * np.stack((np.cos(a), np.sin(a)))
        j = np.argmin(np.hypot(lm[0][:, None] - p[0][None, :], lm[1][:, None] - p[1][None, :]), axis=0)
        scans[:, t] = np.hypot(lm[0, j] - x_true[0, t], lm[1, j] - x_true[1, t])
        scans[beams:, t] = 10.0
    u = np.zeros((2, T))
    u[0] = 0.02
    cfgd = dict(N=1, deltat=0.1, L=4000, Q=[1, 1], R=[1, 1, 1], cte_odom=1.0, cota=1.0, dist_thr=0.09,
                dist_thr_obs=1.0, rango_laser_max=10.0, radio=0.0)
    return lm, scans, x_true, u, cfgd


def test_scan_with_many_distinct_landmarks_grows_the_hash_table():
    """A scan touching > 96 distinct landmarks overflows the default 128-slot per-pose table of
    k_assoc_group; the sweep relaunches phase A with 256 slots and still matches the oracle."""
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from oracle import c_oracle as co
    lm, scans, x_true, u, cfgd = _dense_ring_case()
    cfg = ConfigICM(D=cfgd)
    odo = x_true.copy()
    T = x_true.shape[1]
    eng = SweepEngine(cfg)
    eng.upload(scans, odo, u)
    eng.set_debug(True)
    x = x_true.copy()
    mo, cnt, K = eng.sweep(lm, x, x_true[:, 0], lm.shape[1], "redblack")
    lab = eng.association()[0]
    off = eng.kept_beams()[0]
    per_pose = [len(set(lab[off[t]:off[t + 1]])) for t in range(T)]
    eng.close()
    print("distinct labels per pose:", per_pose)
    assert 96 < max(per_pose) <= 192, "the case must overflow the 128-slot table (and fit the 256-slot one)"
    keptc = co.prefilter(cfg, scans)
    xc = x_true.copy()
    mc, cntc, Kc, _ = co.sweep(cfg, keptc, u, odo, x_true[:, 0], lm, xc, lm.shape[1], "redblack")
    assert K == Kc and np.array_equal(cnt, cntc) and np.abs(mo[:, :K] - mc).max() <= 1e-9
    assert np.abs(x - xc).max() <= 1e-9


def test_sweep_queued_whole_recovers_from_a_table_overflow():
    """The same overflowing case through the sweep that is queued without a host look at phase A's flags: the solves and
    Mapa.filtrar see the overflow on the device and replace nothing, the flags come back with the sweep's one wait, and
    the sweep is repeated the careful way -- by the library (icm_sweep_device) and by a caller of the phase calls
    (ShardedSweep, here with a loop-back exchange at world size 1)."""
    import torch
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.sharded import ShardedSweep
    from oracle import c_oracle as co
    lm, scans, x_true, u, cfgd = _dense_ring_case()
    cfg = ConfigICM(D=cfgd)
    odo = x_true.copy()
    T = x_true.shape[1]
    keptc = co.prefilter(cfg, scans)
    xc = x_true.copy()
    mc, cntc, Kc, _ = co.sweep(cfg, keptc, u, odo, x_true[:, 0], lm, xc, lm.shape[1], "redblack")

    eng = SweepEngine(cfg)
    eng.upload(scans, odo, u)
    eng.set_state(lm, x_true, x_true[:, 0])
    eng.sweep_device("redblack")
    x, mo, cnt, K = eng.get_state()
    eng.close()
    assert K == Kc and np.array_equal(cnt, cntc) and np.abs(mo[:, :K] - mc).max() <= 1e-9 and np.abs(x - xc).max() <= 1e-9

    class Loopback:   # world size 1: the rank's own statistics are the gathered ones
        def gather_stats(self, sw):
            sw.stats[:sw.stride].copy_(sw.stats_send)

        def all_gather(self, buf, rank, count):
            pass

    eng = SweepEngine(cfg)
    eng.upload(scans, odo, u)
    run = ShardedSweep(eng, 0, 1, T, comm=Loopback())
    run.set_state(lm, x_true, x_true[:, 0])
    run.sweep("redblack")
    torch.cuda.synchronize()
    x2, m2, c2, K2 = run.get_state()
    eng.close()
    assert K2 == K and np.array_equal(x2, x) and np.array_equal(m2, mo) and np.array_equal(c2, cnt)


def test_handle_reuse_with_longer_sequence():
    """One handle, a short sequence then a longer one (ICM_ROS re-uploads when its data change)."""
    from icmslam_hip import SweepEngine
    zz, odo, u = dataset()
    init = gold("init_pass.npz")
    eng = SweepEngine(Cfg(cota=20.0))
    outs = []
    for T in (150, 600):
        eng.upload(zz[:, :T], odo[:, :T], u[:, :T])
        x = np.ascontiguousarray(init["x_init"][:, :T]).copy()
        mo, co, K = eng.sweep(init["map_init"], x, odo[:, 0], 11, "redblack")
        outs.append((x, mo[:, :K]))
    eng.close()
    e2 = SweepEngine(Cfg(cota=20.0))
    e2.upload(zz[:, :600], odo[:, :600], u[:, :600])
    x2 = np.ascontiguousarray(init["x_init"][:, :600]).copy()
    mo2, co2, K2 = e2.sweep(init["map_init"], x2, odo[:, 0], 11, "redblack")
    e2.close()
    assert np.array_equal(outs[1][0], x2) and np.array_equal(outs[1][1], mo2[:, :K2])


def test_sequential_chain_folded_and_complete_energy_are_bit_identical():
    """The reference's own order (one dependent chain, scripts/ICM_ROS.py:141-158) walked by one lane with the folded
    energy in the loop (automatic) and with the complete energy there (fold mode 0): same poses, same iteration /
    evaluation counts of every pose, on the real dataset."""
    from icmslam_hip import SweepEngine
    zz, odo, u = dataset()
    init = gold("init_pass.npz")
    eng = SweepEngine(Cfg())
    eng.upload(zz, odo, u)
    eng.set_debug(True)
    eng.set_state(init["map_init"], init["x_init"], odo[:, 0], 11)
    for _ in range(2):
        eng.sweep_device("redblack")
    assert eng.solve_diag()[:, 2].max() > 60             # (the red-black solve reports f, nit, nfev of every pose too)
    eng.close()
    eng = SweepEngine(Cfg())
    eng.upload(zz, odo, u)
    eng.set_debug(True)
    seq = {}
    for fold in (-1, 0):
        eng.set_fold_mode(fold)
        eng.set_state(init["map_init"], init["x_init"], odo[:, 0], 11)
        eng.sweep_device("sequential")
        seq[fold] = (eng.get_state(), eng.solve_diag().copy())
    eng.close()
    for a, b in zip(seq[-1][0], seq[0][0]):
        assert np.array_equal(a, b)
    assert np.array_equal(seq[-1][1][:, 1:], seq[0][1][:, 1:])     # nit, nfev of every pose


def test_fused_two_colour_launch_is_bit_identical():
    """Unsharded red-black sweeps of a long sequence run both colours in one launch (even waves
    wait for the two odd waves that hold their poses' neighbours): same poses and map, bit for
    bit, as one launch per colour, over several sweeps."""
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.synthetic import make_workload
    wl = make_workload(40_000, 4_000, 360)     # long: 64 poses per wave in the one-launch solve
    cfg = ConfigICM(D=wl.config)
    eng = SweepEngine(cfg)
    eng.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
    out = {}
    for fuse in (False, True):
        eng.set_colour_fusion(fuse)
        eng.set_state(wl.map_init, wl.x_init, wl.x0)
        eng.enable_timing(True)
        for _ in range(4):
            eng.sweep_device("redblack")
        launches = eng.kernel_times()["k_solve"][1]
        eng.enable_timing(False)
        assert launches == (4 if fuse else 8)
        out[fuse] = eng.get_state()
    eng.close()
    assert np.array_equal(out[False][0], out[True][0]) and np.array_equal(out[False][1], out[True][1])
    assert out[False][3] == out[True][3] and np.array_equal(out[False][2], out[True][2])
    # a short sequence: the same fusion, 32 poses per wave
    zz, odo, u = dataset()
    init = gold("init_pass.npz")
    e2 = SweepEngine(Cfg())
    e2.upload(zz, odo, u)
    res = {}
    for fuse in (False, True):
        e2.set_colour_fusion(fuse)
        e2.set_state(init["map_init"], init["x_init"], odo[:, 0], 11)
        e2.enable_timing(True)
        for _ in range(3):
            e2.sweep_device("redblack")
        assert e2.kernel_times()["k_solve"][1] == (3 if fuse else 6)
        e2.enable_timing(False)
        res[fuse] = e2.get_state()
    e2.close()
    assert np.array_equal(res[False][0], res[True][0]) and np.array_equal(res[False][1], res[True][1])


def test_snapshot_and_restore_on_the_device():
    """icm_snapshot_state / icm_restore_state: sweeps re-run from a snapshot give the same bits,
    whether the snapshot was taken right after icm_set_state (host-built search grid) or between
    sweeps (map, counters and grid produced on the GPU by the fused Mapa.filtrar)."""
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.synthetic import make_workload
    wl = make_workload(1900, 100, 180)
    eng = SweepEngine(ConfigICM(D=wl.config))
    eng.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
    eng.set_state(wl.map_init, wl.x_init, wl.x0)
    eng.snapshot_state()
    runs = []
    for _ in range(2):
        for _ in range(3):
            eng.sweep_device("redblack")
        runs.append(eng.get_state())
        eng.restore_state()
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)
    # snapshot in the middle of a run
    for _ in range(2):
        eng.sweep_device("redblack")
    eng.snapshot_state()
    mid = eng.get_state()
    for _ in range(2):
        eng.sweep_device("redblack")
    after = eng.get_state()
    eng.restore_state()
    back = eng.get_state()
    for a, b in zip(mid, back):
        assert np.array_equal(a, b)
    for _ in range(2):
        eng.sweep_device("redblack")
    again = eng.get_state()
    eng.close()
    for a, b in zip(after, again):
        assert np.array_equal(a, b)
    # a snapshot does not survive a new upload
    e2 = SweepEngine(ConfigICM(D=wl.config))
    e2.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
    e2.set_state(wl.map_init, wl.x_init, wl.x0)
    from icmslam_hip import IcmError
    with pytest.raises((IcmError, ValueError, RuntimeError)):
        e2.restore_state()
    e2.close()


def _s1_state_after(sweeps, setup):
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.synthetic import WORKLOADS, make_workload
    wl = make_workload(*WORKLOADS["S1"])
    eng = SweepEngine(ConfigICM(D=wl.config))
    eng.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
    setup(eng)
    eng.set_state(wl.map_init, wl.x_init, wl.x0)
    for _ in range(sweeps):
        eng.sweep_device("redblack")
    out = eng.get_state(), eng.fused_deferred()
    eng.close()
    return out


def test_fused_solve_defers_instead_of_depending_on_dispatch_order():
    """The one-launch red-black solve must not need its odd waves to be dispatched first: an even
    wave that does not see its neighbours' flags within the poll budget leaves its poses alone and
    the wave that finishes the launch last solves them (inside the same launch: nothing is queued
    behind a solve launch).  With a budget of 0 polls nearly every even wave takes that road -- the
    result is bit-identical to the default and to one launch per colour (with a budget of 0 polls
    too: nothing to defer there), and the default run defers nothing."""
    (ref, nd_ref) = _s1_state_after(3, lambda e: None)
    (two, _) = _s1_state_after(3, lambda e: e.set_colour_fusion(False))
    (zero, nd_zero) = _s1_state_after(3, lambda e: e.set_fused_spin_limit(0))
    (two0, nd_two0) = _s1_state_after(3, lambda e: (e.set_colour_fusion(False), e.set_fused_spin_limit(0)))
    print("even waves deferred: default %d, 0 polls %d (one launch) / %d (one launch per colour)" % (nd_ref, nd_zero, nd_two0))
    assert nd_ref == 0 and nd_zero > 0 and nd_two0 == 0
    for other in (two, zero, two0):
        for a, b in zip(ref, other):
            assert np.array_equal(a, b)


def test_fused_solve_with_far_more_waves_than_the_chip_holds():
    """1 000 001 poses (15 626 solve waves against at most a few thousand resident): every even
    wave's neighbours were dispatched before it, so the one-launch solve needs no deferral, and it
    equals one launch per colour bit for bit."""
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.synthetic import make_workload
    wl = make_workload(1_000_001, 2500, 180)
    cfg = ConfigICM(D=wl.config)
    eng = SweepEngine(cfg)
    eng.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
    states = []
    for fused in (True, False):
        eng.set_colour_fusion(fused)
        eng.set_state(wl.map_init, wl.x_init, wl.x0)
        for _ in range(2):
            eng.sweep_device("redblack")
        states.append(eng.get_state())
    nd = eng.fused_deferred()
    eng.close()
    print("1M poses: even waves deferred %d" % nd)
    for a, b in zip(*states):
        assert np.array_equal(a, b)
    assert np.isfinite(states[0][0]).all() and nd == 0


def test_three_engines_on_concurrent_streams_equal_their_solo_runs():
    """Three handles (three HIP streams) driven from three host threads at once: the fused solves
    of one engine share the chip with the other engines' kernels, so workgroups of different grids
    interleave arbitrarily -- every sweep must still equal the engine's solo run bit for bit."""
    import threading
    import torch
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.synthetic import make_workload
    wls = [make_workload(30_000, 2_500, 360, seed=20181 + i) for i in range(3)]
    engs = []
    for wl in wls:
        e = SweepEngine(ConfigICM(D=wl.config), 0)
        e.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
        e.set_state(wl.map_init, wl.x_init, wl.x0)
        e.snapshot_state()
        engs.append(e)

    def run(e, rounds, out, k):
        st = []
        for _ in range(rounds):
            for _ in range(5):
                e.sweep_device("redblack")
            st.append(e.get_state()[0].copy())
            e.restore_state()
        out[k] = st

    solo = [None] * 3
    for k, e in enumerate(engs):
        run(e, 1, solo, k)
    torch.cuda.synchronize()
    got = [None] * 3
    th = [threading.Thread(target=run, args=(e, 12, got, k)) for k, e in enumerate(engs)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    torch.cuda.synchronize()
    nd = [e.fused_deferred() for e in engs]
    for e in engs:
        e.close()
    print("concurrent engines: even waves deferred", nd)
    for k in range(3):
        for j, s in enumerate(got[k]):
            assert np.array_equal(s, solo[k][0]), "engine %d round %d differs from its solo run" % (k, j)


def test_rigid_motion_equivariance_at_s1_size():
    """Size-independent property: moving the whole problem (poses, odometry, map) by a rigid
    transform moves the result by the same transform UP TO THE SOLVER'S TOLERANCE -- the
    reference's fmin builds its initial simplex relative to the absolute coordinates (x0 * 1.05),
    so the Nelder-Mead path, and with it the result within xtol = 1e-3 / ftol = 1e-4, depends on
    where the origin is; everything else (search-grid origin and clamping, cell assignment, chunk
    tables, the moment form's expansion point) must not: associations, counts and the landmark
    set are identical, poses and map agree to a few solver tolerances."""
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.synthetic import WORKLOADS, make_workload
    T, K, B = WORKLOADS["S1"]
    wl = make_workload(T, K, B)
    cfg = ConfigICM(D=wl.config)
    phi, shift = 0.7, np.array([[1234.5], [-678.25]])
    Rm = np.array([[np.cos(phi), -np.sin(phi)], [np.sin(phi), np.cos(phi)]])

    def move_pose(p):
        q = np.array(p, dtype=float, copy=True)
        q[:2] = Rm @ p[:2] + (shift if p.ndim == 2 else shift[:, 0])
        q[2] = p[2] + phi
        return q

    def run(odo, x_init, x0, m_init):
        eng = SweepEngine(cfg)
        eng.upload(wl.scans, odo, wl.u, pose_major=True)
        eng.set_state(m_init, x_init, x0)
        for _ in range(2):
            eng.sweep_device("redblack")
        out = eng.get_state()
        eng.close()
        return out

    x_a, m_a, c_a, K_a = run(wl.odometry, wl.x_init, wl.x0, wl.map_init)
    x_b, m_b, c_b, K_b = run(move_pose(wl.odometry), move_pose(wl.x_init), move_pose(wl.x0), Rm @ wl.map_init + shift)
    assert K_a == K_b and np.array_equal(c_a, c_b)
    exp_m = Rm @ m_a[:, :K_a] + shift
    print("rigid motion: max map difference %.3e" % np.abs(m_b[:, :K_b] - exp_m).max())
    assert np.abs(m_b[:, :K_b] - exp_m).max() <= 1e-2
    exp_x = move_pose(x_a)
    d = np.abs(x_b - exp_x)
    d[2] = np.abs(np.angle(np.exp(1j * (x_b[2] - exp_x[2]))))
    dm = d.max(axis=0)
    print("rigid motion: max|dx| %.3e, median %.3e, poses above 5e-3: %d of %d" % (dm.max(), np.median(dm), int((dm > 5e-3).sum()), T))
    assert np.median(dm) <= 2e-3 and dm.max() <= 0.2 and (dm > 5e-3).sum() <= T // 100


def test_pose_table_filling_up_inside_one_fold_does_not_spin():
    """~45 distinct landmarks per 64-beam chunk over three chunks: the 128-slot per-pose table is
    within its 96-label budget after two chunks and would be over-full after the third.  The probe
    loop is bounded, the sweep notices, relaunches phase A with 256 slots and matches the oracle
    (an unbounded probe would spin on the full table)."""
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from oracle import c_oracle as co
    lm, scans, x_true, u, cfgd = _dense_ring_case(grid=0.07, beams=224)
    cfgd = dict(cfgd, dist_thr=0.055, L=14000)
    cfg = ConfigICM(D=cfgd)
    odo = x_true.copy()
    T = x_true.shape[1]
    keptc = co.prefilter(cfg, scans)
    for debug in (False, True):
        eng = SweepEngine(cfg)
        eng.upload(scans, odo, u)
        eng.set_debug(debug)
        x = x_true.copy()
        mo, cnt, K = eng.sweep(lm, x, x_true[:, 0], lm.shape[1], "redblack")
        if debug:
            lab = eng.association()[0]
            off = eng.kept_beams()[0]
            per_pose = [len(set(lab[off[t]:off[t + 1]])) for t in range(T)]
            print("distinct labels per pose:", per_pose)
            assert 128 < max(per_pose) <= 192
        eng.close()
        xc = x_true.copy()
        mc, cntc, Kc, _ = co.sweep(cfg, keptc, u, odo, x_true[:, 0], lm, xc, lm.shape[1], "redblack")
        assert K == Kc and np.array_equal(cnt, cntc) and np.abs(mo[:, :K] - mc).max() <= 1e-9
        assert np.abs(x - xc).max() <= 1e-9


@pytest.mark.timeout(120)
def test_non_finite_inputs_do_not_hang():
    """Garbage in (an infinite landmark coordinate, a NaN pose) may give garbage or an error out,
    but every kernel and host loop must terminate: the grid-sizing loops are bounded, NaN world
    points fall into cell 0 and are gated out."""
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.synthetic import make_workload
    wl = make_workload(1900, 100, 180)
    cfg = ConfigICM(D=wl.config)
    for what in ("inf-landmark", "nan-pose", "inf-pose"):
        m, x = wl.map_init.copy(), wl.x_init.copy()
        if what == "inf-landmark":
            m[0, 7] = np.inf
        elif what == "nan-pose":
            x[:, 500] = np.nan
        else:
            x[0, 900] = np.inf
        eng = SweepEngine(cfg)
        eng.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
        try:
            eng.set_state(m, x, wl.x0)
            for _ in range(3):
                eng.sweep_device("redblack")
            out = eng.get_state()
            print(what, "-> finished; finite poses: %d of %d" % (int(np.isfinite(out[0]).all(axis=0).sum()), wl.T))
        except (IndexError, ValueError, RuntimeError) as e:
            print(what, "-> raised", type(e).__name__, str(e)[:80])
        eng.close()


def test_fold_only_solve_with_fixup_is_bit_identical():
    """The one-launch solve in its fold-only form (13 coefficients per pose in the Nelder-Mead loop; a pose outside
    the folded form's range solved once more by its wave with the complete energy) against the complete energy in the
    loop itself: S1 over 6 sweeps with state reads, snapshot / restore and host-array sweeps in between -- every
    state bit-equal."""
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.synthetic import WORKLOADS, make_workload
    wl = make_workload(*WORKLOADS["S1"])
    cfg = ConfigICM(D=wl.config)

    def run(mode):
        eng = SweepEngine(cfg)
        eng.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
        eng.set_fold_mode(mode)
        eng.set_state(wl.map_init, wl.x_init, wl.x0)
        out = []
        for it in range(6):
            eng.sweep_device("redblack")
            if it == 1:
                eng.snapshot_state()
            if it in (0, 2, 5):
                out.append(eng.get_state())
        eng.restore_state()                      # back to the state after sweep 2 ...
        eng.sweep_device("redblack")             # ... and sweep 3 again
        out.append(eng.get_state())
        x = out[-1][0].copy()                    # a host-array sweep from there (icm_sweep: set_state + sweep + get_state)
        mo, co, K = eng.sweep(out[-1][1][:, :out[-1][3]], x, wl.x0, out[-1][3], "redblack")
        out.append((x, mo, co, K))
        nd, nf = eng.fused_deferred(), eng.fixup_poses()
        eng.close()
        return out, nd, nf

    ref, _, nf0 = run(0)
    got, nd, nf1 = run(1)
    auto, _, nfa = run(-1)
    print("fold-only S1: even waves deferred %d, poses solved a second time %d (automatic mode: %d)" % (nd, nf1, nfa))
    assert nf0 == 0 and nfa == nf1      # isotropic weights: automatic = fold-only
    for a, b, c in zip(ref, got, auto):
        for u, v, w in zip(a, b, c):
            assert np.array_equal(u, v) and np.array_equal(u, w)
    # restore + one sweep reproduces sweep 3 of the straight run
    assert np.array_equal(got[3][0], got[1][0]) and np.array_equal(got[3][1], got[1][1])


def test_fixup_launches_take_poses_outside_the_folded_range():
    """Poses whose heading is off by 0.4 rad start their solve outside the folded form's range (|d theta| <= 0.25):
    the fold-only kernel must solve exactly those -- and whatever their kick pushes out of range around them -- a
    second time with the complete energy, and the sweep must equal the one with the complete energy in the loop
    itself, bit for bit, and the C oracle to 1e-9.  Same with anisotropic weights forced through the fold-only kernel
    (the folded form never holds: every solved pose is solved twice)."""
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.synthetic import make_workload
    from oracle import c_oracle as co
    wl = make_workload(1900, 100, 180)
    for what, Q in (("kicked headings", [1.0, 1.0]), ("anisotropic Q", [1.0, 1.5])):
        conf = dict(wl.config)
        conf["Q"] = Q
        cfg = ConfigICM(D=conf)
        x0 = wl.x_init.copy()
        if what == "kicked headings":
            x0[2, 45:wl.T - 2:50] += 0.4          # odd poses 45, 95, ...
            x0[2, 70:wl.T - 2:100] -= 0.4         # even poses 70, 170, ...
        outs = {}
        for mode in (0, 1):
            eng = SweepEngine(cfg)
            eng.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
            eng.set_fold_mode(mode)
            eng.set_state(wl.map_init, x0, wl.x0)
            for _ in range(2):
                eng.sweep_device("redblack")
            outs[mode] = (eng.get_state(), eng.fixup_poses())
            eng.close()
        (ref, n0), (got, n1) = outs[0], outs[1]
        print("%s: poses solved a second time %d (of %d pose solves)" % (what, n1, 2 * (wl.T - 1)))
        assert n0 == 0
        if what == "kicked headings":
            assert 30 <= n1 < 400                  # the kicked poses and their neighbours, not the sequence
        else:
            assert n1 >= 0.7 * 2 * (wl.T - 1)        # everything but the no-beam odd poses of the turn (they need no energy)
        for u, v in zip(ref, got):
            assert np.array_equal(u, v)
        kept = co.prefilter(cfg, wl.scans.T)
        xc, mv, la = x0.copy(), wl.map_init, wl.K
        for _ in range(2):
            mv, cnt, la, _ = co.sweep(cfg, kept, wl.u, wl.odometry, wl.x0, mv, xc, la, "redblack")
        x, m, c, K = got
        assert K == la and np.array_equal(c, cnt) and np.abs(m[:, :K] - mv).max() <= 1e-9
        d = np.abs(x - xc).max(axis=0)
        print("%s vs C oracle: max|dx| %.3e, poses above 1e-9: %d" % (what, d.max(), int((d > 1e-9).sum())))
        assert d.max() <= 1e-9


def test_fixup_launches_with_deferred_waves_and_per_colour_launches():
    """Both rare roads of the one-launch solve at once: poses outside the folded form's range (solved a second time by
    their wave) and even waves that deferred (solved by the launch's last wave).  With the poll budget at 0 EVERY even
    wave whose odd neighbours are not done at its first look defers; with kicked headings some poses leave the folded
    range on top of that -- and one launch per colour beside it, all against the complete-energy one-launch kernel with
    the default poll budget: bit-identical."""
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.synthetic import make_workload
    wl = make_workload(1900, 100, 180)
    cfg = ConfigICM(D=wl.config)
    x0 = wl.x_init.copy()
    x0[2, 45:wl.T - 2:50] += 0.4
    x0[2, 70:wl.T - 2:100] -= 0.4
    outs = []
    for fold, fuse, spin in ((0, True, None), (1, True, 0), (1, False, 0), (0, False, None)):
        eng = SweepEngine(cfg)
        eng.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
        eng.set_fold_mode(fold)
        eng.set_colour_fusion(fuse)
        if spin is not None:
            eng.set_fused_spin_limit(spin)
        eng.set_state(wl.map_init, x0, wl.x0)
        for _ in range(3):
            eng.sweep_device("redblack")
        outs.append((eng.get_state(), eng.fused_deferred(), eng.fixup_poses()))
        eng.close()
    print("deferred waves / poses solved twice per configuration:", [(o[1], o[2]) for o in outs])
    assert outs[1][1] > 0 and outs[1][2] > 0, "both rare roads were taken in the same launches"
    for o in outs[1:]:
        for a, b in zip(outs[0][0], o[0]):
            assert np.array_equal(a, b)


def test_fold_only_solve_on_the_dataset_sequential_and_redblack():
    """data_IJAC2018: the reference-order sweep (one chain, complete energy) is untouched by the fold-only form; the
    red-black sweeps agree between the two forms of the one-launch solve over three sweeps."""
    from icmslam_hip import SweepEngine
    from util import Cfg, dataset, gold
    zz, odo, u = dataset()
    init = gold("init_pass.npz")
    res = []
    for mode in (0, 1):
        eng = SweepEngine(Cfg())
        eng.upload(zz, odo, u)
        eng.set_fold_mode(mode)
        eng.set_state(init["map_init"], init["x_init"], odo[:, 0], int(init["landmarks_actuales"]))
        for _ in range(3):
            eng.sweep_device("redblack")
        res.append((eng.get_state(), eng.fixup_poses()))
        eng.close()
    print("data_IJAC2018: poses solved a second time over 3 sweeps: %d" % res[1][1])
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b)


def test_host_array_sweeps_reuse_the_device_map_only_when_it_is_the_same_map():
    """icm_sweep keeps the search grid of the last Mapa.filtrar when the caller hands back exactly the
    map it returned (the reference driver's mapa_viejo = copy(mapa_refinado)); any edit of the map --
    here one landmark moved out of reach of its beams -- must reach the device."""
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from icmslam_hip.synthetic import make_workload
    wl = make_workload(1900, 100, 180)
    cfg = ConfigICM(D=wl.config)

    def two_sweeps(edit, fresh_engine_for_second):
        eng = SweepEngine(cfg)
        eng.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
        x = wl.x_init.copy()
        mo, co, K = eng.sweep(wl.map_init, x, wl.x0, wl.K, "redblack")
        mv = mo[:, :K].copy()
        if edit:
            mv[0, 3] += 5.0
        if fresh_engine_for_second:
            eng.close()
            eng = SweepEngine(cfg)
            eng.upload(wl.scans, wl.odometry, wl.u, pose_major=True)
        mo2, co2, K2 = eng.sweep(mv, x, wl.x0, K, "redblack")
        eng.close()
        return x, mo2[:, :K2], co2

    for edit in (False, True):
        a = two_sweeps(edit, False)
        b = two_sweeps(edit, True)
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
    assert not np.array_equal(two_sweeps(False, False)[1], two_sweeps(True, False)[1])
