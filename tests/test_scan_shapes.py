"""The wide-scan scenes of tests/scan_shapes.py on the CPU (no GPU, no HIP): each reaches what it is built for, and the
compiled C oracle -- the reference the GPU tests of test_gpu_scan_shapes.py hold the kernels to at these shapes -- equals
the NumPy oracle there: kept beams bit for bit, one red-black sweep (labels and counters exact, map and poses <= 1e-9)
and the initialisation pass."""
import numpy as np
import pytest

import scan_shapes as ss
from oracle import icm_oracle as o

TOL = 1e-9


def _cfg(sc):
    from ICM_SLAM_tools import ConfigICM
    return ConfigICM(D=sc.config)


def test_wide_ring_reaches_capped_runs_and_three_batches_of_runs():
    for B in (1440, 1462):
        sc = ss.scene("ring", B)
        r = sc.reach
        print(ss.summary(sc))
        assert r["min_margin"] > ss.MARGIN_TOL * sc.thr
        assert r["capped"] > 0, "runs of kRunCap = 64 beams"
        runs = set(r["runs"])
        assert {63, 64, 65, 128, 129}.issubset(runs) and max(runs) > 128, "run counts at and around one and two waves"
        assert {63, 64, 65, 128, 129}.issubset(set(r["kept"])) and max(r["kept"]) == B, "kept beams likewise"
        assert 0 in r["kept"] and r["kept"][0] > 0 and r["kept"][-1] > 0, "empty scans between wide ones"
        assert all(b > 0 for b in r["unsettled_batch"]), "unsettled runs in the first, second and third batch of 64"
        assert all(b > 0 for b in r["settled_batch"]), "settled multi-beam runs in every batch"
        assert max(r["labels"]) <= 96, "fits the 128-slot table: no relaunch"
        assert max(r["labels"]) > 64 and any(r["fresh"]), "more than 64 entries in a pose; gated-out beams make fresh labels"
        assert all(sc.reach["runs"][t] > 64 and sc.reach["multi_beam_runs"][t] > 64 for t in ss.GHOSTS_96), \
            "the ghost scans of 2 and 3 shards hold more than 64 multi-beam runs"


def test_dense_ring_reaches_the_relaunch_with_multi_beam_runs():
    for B in (1440, 1462):
        sc = ss.scene("dense", B)
        r = sc.reach
        print(ss.summary(sc))
        assert r["min_margin"] > ss.MARGIN_TOL * sc.thr
        assert 96 < max(r["labels"]) <= 192, "overflows the 128-slot table, fits the 256-slot one"
        wide = [t for t, n in enumerate(r["labels"]) if n > 96]
        assert all(r["multi_beam_runs"][t] > 64 for t in wide), "with multi-beam runs"
        assert r["capped"] > 0


@pytest.mark.parametrize("B", [64, 65])
def test_small_rings_reach_one_wave_of_runs(B):
    sc = ss.scene("ring", B)
    r = sc.reach
    print(ss.summary(sc))
    assert r["min_margin"] > ss.MARGIN_TOL * sc.thr
    assert max(r["runs"]) == B and max(r["kept"]) == B and 0 in r["kept"]
    assert B - 2 in r["runs"] and r["unsettled"] > 0 and any(r["fresh"])


def test_trunks_reach_more_than_128_kept_beams_per_scan_with_many_labels():
    sc = ss.scene("trunks", 1440)
    r = sc.reach
    print(ss.summary(sc))
    assert max(r["kept"]) > 128 and sum(n > 128 for n in r["kept"]) > sc.T // 3 and 0 in r["kept"]
    assert r["kept"][0] > 128 and r["labels"][0] > 32


@pytest.mark.parametrize("kind,B", [("ring", 64), ("ring", 65), ("ring", 1440), ("ring", 1462), ("trunks", 1440)])
def test_c_oracle_prefilter_equals_numpy_oracle(kind, B):
    from oracle import c_oracle as co
    sc = ss.scene(kind, B)
    cfg = _cfg(sc)
    off, k, d, ang, bx, by = co.prefilter(cfg, sc.ranges)
    kept = o.prefilter_all(sc.ranges, ss.oracle_config(sc))
    n = np.array([kz.shape[0] if kz.ndim == 2 else 0 for kz in kept])
    assert np.array_equal(np.diff(off), n)
    rows = np.concatenate([kz for kz in kept if kz.ndim == 2 and kz.shape[0]])
    assert np.array_equal(d, rows[:, 0]) and np.array_equal(ang, rows[:, 1])
    assert np.array_equal(bx, rows[:, 2]) and np.array_equal(by, rows[:, 3])


@pytest.mark.parametrize("kind,B", [("ring", 1440), ("dense", 1462), ("ring", 65)])
def test_c_oracle_sweep_equals_numpy_oracle(kind, B):
    """One red-black sweep from the scene's state: labels of every kept beam and targets, counters and K exact; map and
    poses <= 1e-9."""
    from oracle import c_oracle as co
    sc = ss.scene(kind, B)
    cfg = _cfg(sc)
    keptc = co.prefilter(cfg, sc.ranges)
    xc = sc.x_init.copy()
    a = {}
    mc, cntc, Kc, (yr, cr, lr) = co.sweep(cfg, keptc, sc.u, sc.odometry, sc.x0, sc.map, xc, sc.map.shape[1], "redblack", assoc=a)
    ocfg = ss.oracle_config(sc)
    st = o.MapState(ocfg, sc.map.shape[1])
    xn = sc.x_init.copy()
    labs = []
    mn, xn = o.sweep(ocfg, st, sc.ranges, sc.u, sc.odometry, sc.x0, sc.map.copy(), xn, schedule="redblack",
                     trace=lambda t, c, tg, xt: labs.append((t, c)))
    off = keptc[0]
    lab = a["labels"]
    lact0 = sc.map.shape[1]
    for t, c in labs:
        # (the NumPy oracle traces every solved pose's labels after its fresh id is given out; the C oracle the same ids)
        assert np.array_equal(lab[off[t]:off[t + 1]], c), "labels of pose %d" % t
    assert Kc == mn.shape[1] == st.landmarks_actuales
    assert np.array_equal(cntc[:Kc], st.cant_obs_i[:Kc])
    dm, dx = np.abs(mc - mn).max(), np.abs(xc - xn).max()
    print("%s B=%d: %d poses, %d beams, K %d -> %d (fresh ids from %d), C vs NumPy: max|dmap| %.2e max|dx| %.2e"
          % (kind, B, sc.T, int(off[-1]), lact0, Kc, lact0, dm, dx))
    assert dm <= TOL and dx <= TOL


def test_c_oracle_init_pass_equals_numpy_oracle():
    from oracle import c_oracle as co
    sc = ss.scene("trunks", 1440)
    cfg = _cfg(sc)
    ocfg = ss.oracle_config(sc)
    keptn = o.prefilter_all(sc.ranges, ocfg)
    st = o.MapState(ocfg)
    y0, _ = o.cluster_first_scan(st, np.zeros((2, ocfg.L)), o.project_beams(sc.odometry[:, 0].copy(), keptn[0][:, 2:4]))
    xc, yc, cc, lc = co.init_pass(cfg, co.prefilter(cfg, sc.ranges), sc.u, sc.odometry, y0, st.cant_obs_i, st.landmarks_actuales)
    # (the NumPy pass ends with Mapa.filtrar, which -- like the reference -- needs some landmark below cota: the raw
    # outputs compared here come before it)
    assert cc[:lc].min() < cc[:lc].max()
    ocfg.cota = cc[:lc].min() + 0.5
    xn, mn, stn, c0, (yn, cn, ln) = o.init_pass(ocfg, sc.ranges, sc.u, sc.odometry, kept=keptn)
    print("trunks init pass: %d clusters in scan 0, %d labels raw; C vs NumPy: max|dx| %.2e max|dy| %.2e"
          % (int(c0.max()) + 1, lc, np.abs(xc - xn).max(), np.abs(yc - yn).max()))
    assert lc == ln and np.array_equal(cc, cn)
    assert np.abs(yc - yn).max() <= TOL and np.abs(xc - xn).max() <= TOL


def test_header_states_the_beam_limit_the_prefilter_staging_sets():
    """include/icmslam.h's ICM_MAX_BEAMS is what k_prefilter's LDS staging holds: 4 waves x B x (3 doubles + 1 int) of
    the 160 KiB one workgroup may take (the library static_asserts the same; tests/test_gpu_scan_shapes.py checks the
    refusal at upload)."""
    import os
    import re
    from util import ROOT
    h = open(os.path.join(ROOT, "include", "icmslam.h")).read()
    limit = int(re.search(r"#define ICM_MAX_BEAMS (\d+)", h).group(1))
    assert limit == 160 * 1024 // (4 * (3 * 8 + 4)) == 1462
    assert max(ss.scene("ring", limit).reach["kept"]) == limit, "the scenes reach the limit itself"
