"""Many independent sequences at once (icm_init_pass_batch / icm_sweep_batch, k_init_pass_batch,
k_solve_m_sequential_batch, icmslam_hip.batch): every member bit for bit what its own single call gives.

Members (mixed throughout): data_IJAC2018 at the default config; the same at dist_thr = 0.7; with anisotropic Q / R
(the complete-energy chain launch beside the folded one); cut to T = 500; a synthetic sequence at B = 360; a wide-scan
scene at B = 1440 (its LDS need is not the first member's).
"""
import ctypes as C
import os

import numpy as np
import pytest

from util import GOLD, dataset, gold

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _cfg(**kw):
    from ICM_SLAM_tools import ConfigICM
    cfg = ConfigICM("config_default.yaml")
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _specs():
    """name -> (config, upload args, upload kwargs, x0)."""
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip.synthetic import make_workload
    import scan_shapes
    zz, odo, u = dataset()
    out = {
        "ijac": (_cfg(), (zz, odo, u), {}, odo[:, 0]),
        "thr07": (_cfg(dist_thr=0.7), (zz, odo, u), {}, odo[:, 0]),
        "aniso": (_cfg(Q=np.diag([2.0, 0.5]), R=np.diag([1.5, 0.7, 2.0])), (zz, odo, u), {}, odo[:, 0]),
        "t500": (_cfg(), (zz[:, :500], odo[:, :500], u[:, :500]), {}, odo[:, 0]),
    }
    wl = make_workload(600, 64, 360)
    out["synth"] = (ConfigICM(D=wl.config), (wl.scans, wl.odometry, wl.u), {"pose_major": True}, wl.odometry[:, 0])
    sc = scan_shapes.scene("ring", 1440)
    out["wide"] = (ConfigICM(D=sc.config), (sc.ranges, sc.odometry, sc.u), {}, sc.odometry[:, 0])
    return out


SPECS = None


def specs():
    global SPECS
    if SPECS is None:
        SPECS = _specs()
    return SPECS


def _engine(name, **cfg_kw):
    from icmslam_hip import SweepEngine
    cfg, args, kw, _ = specs()[name]
    if cfg_kw:
        import copy
        cfg = copy.copy(cfg)
        for k, v in cfg_kw.items():
            setattr(cfg, k, v)
    e = SweepEngine(cfg)
    e.upload(*args, **kw)
    return e


def _same(a, b):
    """Two results of init_pass (tuples of arrays / ints) or two exceptions are identical."""
    if isinstance(a, Exception) or isinstance(b, Exception):
        return type(a) is type(b) and str(a) == str(b)
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def _single_init(e, x0):
    try:
        return e.init_pass(x0)
    except Exception as ex:   # noqa: BLE001
        return ex


def _filtered(cfg, r):
    """inicializar_offline's Mapa.filtrar of an init-pass result: (mapa (2,K), x, K, cant_obs_i)."""
    from ICM_SLAM_tools import Mapa
    x, y, cnt, lact, _ = r
    mo = Mapa(cfg)
    mo.landmarks_actuales = lact
    mo.cant_obs_i = cnt
    yy = mo.filtrar(y)[:, :mo.landmarks_actuales]
    return yy.copy(), x.copy(), mo.landmarks_actuales, mo.cant_obs_i


def _pair(names):
    """Batch engines and their twins, both with the same state (the single init pass + Mapa.filtrar)."""
    bat, twin = [], []
    for n in names:
        cfg, _, _, x0 = specs()[n]
        a, b = _engine(n), _engine(n)
        mapa, x, K, _ = _filtered(cfg, b.init_pass(x0))
        for e in (a, b):
            e.set_state(mapa, x, x0, K)
        bat.append(a)
        twin.append(b)
    return bat, twin


def _states_equal(a, b):
    sa, sb = a.get_state(), b.get_state()
    return all(np.array_equal(p, q) for p, q in zip(sa, sb))


def _close(*groups):
    for g in groups:
        for e in g:
            e.close()


NAMES = ["ijac", "thr07", "aniso", "t500", "synth", "wide"]


def test_init_pass_batch_bit_for_bit():
    from icmslam_hip import init_pass_batch
    bat = [_engine(n) for n in NAMES]
    twin = [_engine(n) for n in NAMES]
    x0s = [specs()[n][3] for n in NAMES]
    got = init_pass_batch(bat, x0s)
    for n, e, x0, r in zip(NAMES, twin, x0s, got):
        want = _single_init(e, x0)
        assert not isinstance(want, Exception), (n, want)
        assert _same(r, want), n
    # the dataset member after Mapa.filtrar against the reference's init pass
    mapa, x, K, cnt = _filtered(specs()["ijac"][0], got[0])
    g = gold("init_pass.npz")
    assert mapa.shape == g["map_init"].shape
    assert np.abs(mapa - g["map_init"]).max() <= TOL
    assert np.abs(x - g["x_init"]).max() <= TOL
    assert np.array_equal(cnt, g["cant_obs_i"])
    _close(bat, twin)


def test_init_pass_batch_failing_member():
    from icmslam_hip import init_pass_batch
    x0 = specs()["ijac"][3]
    probe = _engine("ijac")
    ncl = int(probe.init_pass(x0)[4].max()) + 1   # clusters of scan 0
    probe.close()
    names = ["thr07", "small", "synth", "wide"]

    def make(n):
        return _engine("ijac", L=ncl + 1) if n == "small" else _engine(n)
    bat = [make(n) for n in names]
    twin = [make(n) for n in names]
    x0s = [specs()["ijac" if n == "small" else n][3] for n in names]
    got = init_pass_batch(bat, x0s)
    for n, e, x0, r in zip(names, twin, x0s, got):
        want = _single_init(e, x0)
        if n == "small":
            assert isinstance(want, IndexError) and isinstance(r, IndexError)
            assert str(r) == str(want)
        else:
            assert not isinstance(want, Exception), (n, want)
            assert _same(r, want), n
    _close(bat, twin)


def test_sweep_batch_three_sweeps_bit_for_bit():
    from icmslam_hip import sweep_batch
    bat, twin = _pair(NAMES)
    for it in range(3):
        res = sweep_batch(bat)
        assert res == [None] * len(NAMES), res
        for n, a, b in zip(NAMES, bat, twin):
            b.sweep_device("sequential")
            assert _states_equal(a, b), "%s after sweep %d" % (n, it + 1)
    _close(bat, twin)


def test_sweep_batch_then_single_sweeps():
    """A batched sweep leaves the bookkeeping a single one leaves: the next single sweeps of either schedule agree."""
    from icmslam_hip import sweep_batch
    names = ["ijac", "aniso", "synth"]
    bat, twin = _pair(names)
    assert sweep_batch(bat) == [None] * len(names)
    for a, b in zip(bat, twin):
        b.sweep_device("sequential")
    for sched in ("sequential", "redblack"):
        for n, a, b in zip(names, bat, twin):
            a.sweep_device(sched)
            b.sweep_device(sched)
            assert _states_equal(a, b), "%s, then %s" % (n, sched)
    _close(bat, twin)


def test_sweep_batch_order_and_size():
    from icmslam_hip import sweep_batch
    bat, twin = _pair(NAMES)
    perm = [4, 1, 5, 0, 3, 2]
    assert sweep_batch([twin[i] for i in perm]) == [None] * len(NAMES)
    assert sweep_batch(bat) == [None] * len(NAMES)
    for n, a, b in zip(NAMES, bat, twin):
        assert _states_equal(a, b), n
    # a batch of one is the single call
    for n, a, b in zip(NAMES, bat, twin):
        assert sweep_batch([a]) == [None]
        b.sweep_device("sequential")
        assert _states_equal(a, b), n
    _close(bat, twin)


def test_run_offline_reference_parity():
    from ICM_ROS import ICM_ROS
    from icmslam_hip import run_offline
    m = ICM_ROS(_cfg())
    m.load_data(os.path.join(GOLD, "data_IJAC2018.npz"))
    m.inicializar_offline()
    mv, x = m.mapa_viejo.copy(), m.positions.copy()
    loop = []
    for _ in range(2):
        mv, x = m.iterations_process_offline(mv, x)
        mv = mv.copy()
        loop.append((mv.copy(), x.copy()))
    thr = _cfg(dist_thr=0.7)
    probs = [(m.config, m.mediciones, m.odometria, m.u), (thr, m.mediciones, m.odometria, m.u)]
    for n in (1, 2):
        res = run_offline(probs, sweeps=n)
        mapa, xx = res[0]
        g = gold("sweep%02d.npz" % n)
        assert mapa.shape == g["mapa"].shape
        assert np.abs(mapa - g["mapa"]).max() <= TOL
        assert np.abs(xx - g["x"]).max() <= TOL
        assert np.array_equal(mapa, loop[n - 1][0]) and np.array_equal(xx, loop[n - 1][1])
        assert not isinstance(res[1], Exception)
    # the default number of sweeps is config.N of the first member
    res = run_offline(probs[:1])
    assert np.array_equal(res[0][0], loop[m.config.N - 1][0])


def _raw(engines):
    from icmslam_hip import _lib
    lib = _lib.load()
    hs = (C.c_void_p * len(engines))(*[e.h.value for e in engines])
    rcs = (C.c_int32 * len(engines))(*([7] * len(engines)))
    return lib.icm_sweep_batch(hs, len(engines), 0, rcs), list(rcs)


def test_sweep_batch_refusals_leave_state():
    from icmslam_hip import _lib, sweep_batch
    names = ["ijac", "synth"]
    bat, twin = _pair(names)
    fresh = _engine("t500")   # uploaded, no state
    before = [e.get_state() for e in bat]

    def unchanged():
        for e, s in zip(bat, before):
            assert all(np.array_equal(p, q) for p, q in zip(e.get_state(), s))

    with pytest.raises(ValueError):
        sweep_batch([bat[0], bat[1], bat[0]])
    rc, rcs = _raw([bat[0], bat[1], bat[0]])   # the library refuses it on its own, too, and writes no rc_out
    assert rc == _lib.ICM_ERR_ARG and rcs == [7, 7, 7]
    unchanged()
    with pytest.raises(ValueError):
        sweep_batch([])
    with pytest.raises(ValueError):
        sweep_batch([bat[0], fresh])
    rc, rcs = _raw([bat[0], fresh])
    assert rc == _lib.ICM_ERR_ARG and rcs == [7, 7]
    unchanged()
    bat[1].set_energy_form(1)
    with pytest.raises(NotImplementedError):
        sweep_batch(bat)
    bat[1].set_energy_form(0)
    unchanged()
    with pytest.raises(NotImplementedError):
        sweep_batch(bat, "redblack")
    unchanged()
    # and the batch still works afterwards
    assert sweep_batch(bat) == [None, None]
    for n, a, b in zip(names, bat, twin):
        b.sweep_device("sequential")
        assert _states_equal(a, b), n
    _close(bat, twin, [fresh])


def test_wider_batch_64_members():
    from icmslam_hip import SweepEngine, init_pass_batch, sweep_batch
    zz, odo, u = dataset()
    thrs = np.linspace(0.8, 1.2, 64)
    bat, twin = [], []
    for t in thrs:
        for group in (bat, twin):
            e = SweepEngine(_cfg(dist_thr=float(t)))
            e.upload(zz, odo, u)
            group.append(e)
    x0 = odo[:, 0]
    got = init_pass_batch(bat, [x0] * 64)
    for i, (e, r) in enumerate(zip(twin, got)):
        want = e.init_pass(x0)
        assert _same(r, want), i
        mapa, x, K, _ = _filtered(e.config, want)
        bat[i].set_state(mapa, x, x0, K)
        e.set_state(mapa, x, x0, K)
    for it in range(2):
        assert sweep_batch(bat) == [None] * 64
        for e in twin:
            e.sweep_device("sequential")
    for i, (a, b) in enumerate(zip(bat, twin)):
        assert _states_equal(a, b), "dist_thr %.4f" % thrs[i]
    _close(bat, twin)
