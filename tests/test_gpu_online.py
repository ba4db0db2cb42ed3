"""The online initialisation (icm_online_*, k_init_advance, SweepEngine.online_*, ICM_ROS.online_step): a sequence that
grows on the GPU while the causal pass resumes on it.

chunked pass          pushed and advanced in chunks of 1, 3, 64, 1000 and a random mix, from a capacity of 1 (the
                      buffers grow many times): poses, raw map, counts, lact bit for bit == SweepEngine.init_pass;
                      after Mapa.filtrar within 1e-9 of the reference's init pass
push / advance        everything pushed, then advanced to several t_end: the same bits; an empty advance is a no-op
finish                kept beams, runs and two sweeps (both schedules) of the finished handle == a fresh upload's
wide scans            the trunks scene at B = 1440 in uneven chunks == init_pass, and the C oracle within 1e-9
errors                a small L fails at the same sample as the prefix of a larger-L run says; call-order errors
message path          matlab2ros.replay -> ICM.lidar / ICM.odom -> online_step -> online_finish -> two sweeps ==
                      load_messages + inicializar_offline + the same sweeps, without a second upload
"""
import ctypes as C

import numpy as np
import pytest

from util import Cfg, dataset, gold

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _engine(cfg=None):
    from icmslam_hip import SweepEngine
    return SweepEngine(cfg or Cfg())


def _run_online(eng, zz, odo, u, chunks, capacity=1):
    """Push and advance `chunks` (sizes) of the sequence; returns (state, poses the advances returned)."""
    eng.online_begin(zz.shape[0], capacity=capacity, x0=odo[:, 0])
    t, got = 0, [np.asarray(odo[:, :1], dtype=np.float64)]
    for n in chunks:
        eng.online_push(zz[:, t:t + n], odo[:, t:t + n], u[:, t:t + n])
        got.append(eng.online_advance())
        t += n
    assert t == zz.shape[1]
    return eng.online_state(), np.concatenate(got, axis=1)


def _chunks(T, kind, seed=7):
    if kind == "mix":
        rng = np.random.default_rng(seed)
        out = []
        while sum(out) < T:
            out.append(int(rng.choice([1, 2, 5, 17, 64, 200, 333])))
        out[-1] -= sum(out) - T
        return [n for n in out if n > 0]
    return [kind] * (T // kind) + ([T % kind] if T % kind else [])


@pytest.fixture(scope="module")
def whole():
    """init_pass over the uploaded dataset."""
    zz, odo, u = dataset()
    eng = _engine()
    eng.upload(zz, odo, u)
    res = eng.init_pass(odo[:, 0])
    eng.close()
    return res


def _same(a, b):
    xa, ya, ca, la, c0a = a
    xb, yb, cb, lb, c0b = b
    assert xa.shape == xb.shape and np.array_equal(xa, xb), "poses"
    assert np.array_equal(ya, yb), "raw map"
    assert np.array_equal(ca, cb), "counts"
    assert la == lb, "landmarks_actuales"
    assert np.array_equal(c0a, c0b), "clusters of scan 0"


@pytest.mark.parametrize("chunk", [1, 3, 64, 1000, "mix"])
def test_chunked_online_pass_equals_the_whole_pass(whole, chunk):
    from ICM_SLAM_tools import Mapa
    zz, odo, u = dataset()
    eng = _engine()
    st, got = _run_online(eng, zz, odo, u, _chunks(zz.shape[1], chunk))
    eng.close()
    _same(st, whole)
    assert np.array_equal(got[:, 1:], st[0][:, 1:]), "poses returned by the advances"
    # after Mapa.filtrar: the reference's init pass
    cfg = Cfg()
    m = Mapa(cfg)
    m.landmarks_actuales, m.cant_obs_i = st[3], st[2].copy()
    yy = m.filtrar(st[1])[:, :m.landmarks_actuales]
    g = gold("init_pass.npz")
    assert yy.shape == g["map_init"].shape and np.abs(yy - g["map_init"]).max() <= TOL
    assert np.abs(st[0] - g["x_init"]).max() <= TOL
    assert np.array_equal(m.cant_obs_i, g["cant_obs_i"])


def test_push_and_advance_are_decoupled(whole):
    zz, odo, u = dataset()
    T = zz.shape[1]
    eng = _engine()
    eng.online_begin(zz.shape[0], capacity=1)
    eng.online_push(zz[:, :1], odo[:, :1], u[:, :1])
    eng.online_push(zz[:, 1:], odo[:, 1:], u[:, 1:])
    parts = [odo[:, :1].copy()]
    for t_end in (1, 2, 7, 7, 300, 301, 1500, T, T):
        x = eng.online_advance(t_end)
        assert x.shape == (3, t_end - sum(p.shape[1] for p in parts))
        parts.append(x)
    assert eng.online_advance().shape == (3, 0)          # nothing new: a no-op
    st = eng.online_state()
    eng.close()
    _same(st, whole)
    assert np.array_equal(np.concatenate(parts, axis=1)[:, 1:], st[0][:, 1:])


def _fresh(zz, odo, u, cfg=None):
    eng = _engine(cfg)
    eng.upload(zz, odo, u)
    return eng


def test_kept_beams_and_runs_after_finish():
    zz, odo, u = dataset()
    eng = _engine()
    _run_online(eng, zz, odo, u, _chunks(zz.shape[1], "mix", seed=3))
    eng.online_finish()
    ref = _fresh(zz, odo, u)
    assert (eng.T, eng.nloc, eng.nnz) == (ref.T, ref.nloc, ref.nnz)
    for a, b in zip(eng.kept_beams(), ref.kept_beams()):
        assert np.array_equal(a, b)
    assert eng.run_counts() == ref.run_counts()
    for a, b in zip(eng.runs(), ref.runs()):
        assert np.array_equal(a, b)
    eng.close()
    ref.close()


def _two_sweeps(eng, x, m, x0, schedule):
    eng.set_state(m, x, x0)
    for _ in range(2):
        eng.sweep_device(schedule)
    return eng.get_state()


@pytest.mark.parametrize("schedule", ["redblack", "sequential"])
@pytest.mark.parametrize("data", ["dataset", "synthetic"])
def test_sweeps_after_finish_equal_a_fresh_upload(schedule, data):
    if data == "dataset":
        zz, odo, u = dataset()
        cfg = Cfg()
        g = gold("init_pass.npz")
        x, m, x0 = g["x_init"], g["map_init"], odo[:, 0]
    else:
        from ICM_SLAM_tools import ConfigICM
        from icmslam_hip.synthetic import WORKLOADS, make_workload
        wl = make_workload(*WORKLOADS["tiny"])
        cfg = ConfigICM(D=wl.config)
        zz, odo, u = np.ascontiguousarray(wl.scans.T), wl.odometry, wl.u
        x, m, x0 = wl.x_init, wl.map_init, wl.x0
    eng = _engine(cfg)
    _run_online(eng, zz, odo, u, _chunks(zz.shape[1], "mix", seed=11), capacity=16)
    eng.online_finish()
    a = _two_sweeps(eng, x.copy(), m.copy(), x0, schedule)
    ref = _fresh(zz, odo, u, cfg)
    b = _two_sweeps(ref, x.copy(), m.copy(), x0, schedule)
    eng.close()
    ref.close()
    assert a[3] == b[3] and a[3] > 0
    for p, q in zip(a[:3], b[:3]):
        assert np.array_equal(p, q)
    # the drop-in call on the finished handle as well
    e2 = _engine(cfg)
    _run_online(e2, zz, odo, u, [zz.shape[1]])
    e2.online_finish()
    xa = np.ascontiguousarray(x, dtype=np.float64).copy()
    ra = e2.sweep(m, xa, x0, m.shape[1], schedule)
    e3 = _fresh(zz, odo, u, cfg)
    xb = np.ascontiguousarray(x, dtype=np.float64).copy()
    rb = e3.sweep(m, xb, x0, m.shape[1], schedule)
    e2.close()
    e3.close()
    assert np.array_equal(xa, xb) and ra[2] == rb[2]
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])


def test_wide_and_sparse_scans_in_uneven_chunks():
    import scan_shapes as ss
    from ICM_SLAM_tools import ConfigICM
    from oracle import c_oracle as co
    from oracle import icm_oracle as o
    sc = ss.scene("trunks", 1440)
    cfg = ConfigICM(D=sc.config)
    x0 = sc.odometry[:, 0].copy()
    ref = _engine(cfg)
    ref.upload(sc.ranges, sc.odometry, sc.u)
    whole = ref.init_pass(x0)
    ref.close()
    eng = _engine(cfg)
    T = sc.ranges.shape[1]
    chunks = [1, 2, 13, 5, 30]
    chunks.append(T - sum(chunks))
    st, _ = _run_online(eng, sc.ranges, sc.odometry, sc.u, chunks)
    eng.close()
    _same(st, whole)
    n = np.array(sc.reach["kept"])
    assert n.max() > 128 and (n == 0).any()
    ocfg = ss.oracle_config(sc)
    kept = o.prefilter_all(sc.ranges, ocfg)
    ost = o.MapState(ocfg)
    y0, _ = o.cluster_first_scan(ost, np.zeros((2, ocfg.L)), o.project_beams(x0, kept[0][:, 2:4]))
    xc, yc, cc, lc = co.init_pass(cfg, co.prefilter(cfg, sc.ranges), sc.u, sc.odometry, y0, ost.cant_obs_i, ost.landmarks_actuales)
    x, y, cnt, lact, _ = st
    assert lact == lc and np.array_equal(cnt, cc)
    assert np.abs(x - xc).max() <= TOL and np.abs(y - yc).max() <= TOL


def test_map_capacity_error_reports_the_failing_sample():
    zz, odo, u = dataset()
    small = Cfg(L=20)
    ref = _fresh(zz, odo, u, small)
    with pytest.raises(IndexError):
        ref.init_pass(odo[:, 0])
    ref.close()
    eng = _engine(small)
    eng.online_begin(zz.shape[0], capacity=1)
    with pytest.raises(IndexError):
        for t in range(0, zz.shape[1], 50):
            eng.online_push(zz[:, t:t + 50], odo[:, t:t + 50], u[:, t:t + 50])
            eng.online_advance()
    x, y, cnt, lact, _ = eng.online_state()
    t_fail = x.shape[1]
    with pytest.raises(IndexError):                        # (it stays stuck there)
        eng.online_advance()
    assert eng.online_state()[0].shape[1] == t_fail
    eng.close()
    assert lact == 20 and 1 < t_fail < zz.shape[1]
    big = _engine()
    big.online_begin(zz.shape[0], capacity=1)
    big.online_push(zz, odo, u)
    big.online_advance(t_fail)
    xb, yb, cb, lb, _ = big.online_state()
    assert lb == 20
    assert np.array_equal(x, xb) and np.array_equal(y, yb[:, :20]) and np.array_equal(cnt, cb[:20])
    big.online_advance(t_fail + 1)
    assert big.online_state()[3] == 21                     # sample t_fail is where the 21st landmark appears
    big.close()


def test_call_order_errors_leave_the_handle_usable(whole):
    from icmslam_hip import _lib
    zz, odo, u = dataset()
    T = zz.shape[1]
    eng = _engine()
    lib, h = eng.lib, eng.h
    dp = _lib.dptr
    rows = np.ascontiguousarray(zz[:, :10].T)
    o10, u10 = np.ascontiguousarray(odo[:, :10]), np.ascontiguousarray(u[:, :10])
    xb = np.zeros((3, T))

    def refused(rc):
        assert rc == _lib.ICM_ERR_ARG and lib.icm_last_error(h)

    refused(lib.icm_online_push(h, dp(rows), dp(o10), dp(u10), 10, None))               # push before begin
    refused(lib.icm_online_advance(h, 1, dp(xb), None))                                  # advance before begin
    refused(lib.icm_online_finish(h))
    stats = np.zeros(8)                                                                  # a sharded handle
    assert lib.icm_bind_exchange(h, C.c_void_p(stats.ctypes.data), 0, 2) == 0
    cosb, sinb = np.cos(np.arange(181) * np.pi / 180), np.sin(np.arange(181) * np.pi / 180)
    refused(lib.icm_online_begin(h, dp(cosb), dp(sinb), 181, 16))
    assert lib.icm_bind_exchange(h, None, 0, 1) == 0
    assert lib.icm_online_begin(h, dp(cosb), dp(sinb), 100000, 16) == _lib.ICM_ERR_UNSUPPORTED
    eng.online_begin(zz.shape[0], capacity=1)
    refused(lib.icm_online_advance(h, 1, dp(xb), None))                                  # before the seed
    refused(lib.icm_online_seed(h, dp(odo[:, 0].copy()), dp(np.zeros((2, 1000))), dp(np.zeros(1000)), 1))   # before scan 0
    eng.online_push(zz[:, :10], odo[:, :10], u[:, :10])
    refused(lib.icm_online_advance(h, 11, dp(xb), None))                                 # past the pushed samples
    g = gold("init_pass.npz")
    x0 = odo[:, 0].copy()
    refused(lib.icm_set_state(h, dp(g["x_init"].copy()), dp(x0), dp(g["map_init"].copy()), 11, 11))   # sweeps before finish
    refused(lib.icm_sweep_device(h, 1))
    m, c, k = np.zeros((2, 1000)), np.zeros(1000), C.c_int64(0)
    refused(lib.icm_sweep(h, dp(xb), dp(x0), dp(g["map_init"].copy()), 11, 11, 1, dp(m), dp(c), C.byref(k)))
    eng.online_advance()
    eng.online_push(zz[:, 10:], odo[:, 10:], u[:, 10:])
    eng.online_advance()
    _same(eng.online_state(), whole)
    eng.online_finish()
    refused(lib.icm_online_push(h, dp(rows), dp(o10), dp(u10), 10, None))               # push after finish
    refused(lib.icm_online_finish(h))
    eng.set_state(g["map_init"], g["x_init"], x0)                                        # the handle sweeps
    eng.sweep_device("redblack")
    eng.close()


def test_scan_zero_without_beams_raises_as_init_pass_does():
    zz, odo, u = dataset()
    zz = zz.copy()
    zz[:, 0] = Cfg().rango_laser_max
    ref = _fresh(zz, odo, u)
    with pytest.raises(ValueError):
        ref.init_pass(odo[:, 0])
    ref.close()
    eng = _engine()
    eng.online_begin(zz.shape[0], capacity=4)
    with pytest.raises(ValueError):
        eng.online_push(zz[:, :5], odo[:, :5], u[:, :5])
    eng.close()


def test_message_path_drives_the_same_pipeline(monkeypatch):
    from ICM_ROS import ICM_ROS
    from ICM_SLAM_tools import ConfigICM
    from icmslam_hip import SweepEngine
    from matlab2ros.replay import replay
    from sensors_definitions import Lidar, Odometria
    d = gold("data_IJAC2018.npz")
    T = 400
    cfg = ConfigICM("config_default.yaml")
    cfg.cota = 40.0
    obs, od, ve = d["observations"][:, :T], d["odometry"][:, :T], d["velocities"][:, :T]
    # online: one step after every sample's messages
    a = ICM_ROS(cfg)
    steps = []
    replay(obs, od, ve, lambda m: (a.lidar.callback(m), steps.append(a.online_step())), a.odom.callback)
    assert sum(steps) == T and a.dropped_samples == 0
    a.online_finish()
    assert a.iterations_flag
    names = ("mediciones", "odometria", "u", "x0", "mapa_viejo", "positions")
    init_a = {k: getattr(a, k).copy() for k in names}
    init_a["cant_obs_i"], init_a["lact"] = a.mapa_obj.cant_obs_i.copy(), a.mapa_obj.landmarks_actuales
    uploads = []
    real_upload = SweepEngine.upload
    monkeypatch.setattr(SweepEngine, "upload", lambda self, *k, **kw: (uploads.append(1), real_upload(self, *k, **kw))[1])
    res_a = []
    mv, x = a.mapa_viejo.copy(), a.positions.copy()
    for _ in range(2):
        mv, x = a.iterations_process_offline(mv, x)
        res_a.append((mv.copy(), x.copy()))
    assert not uploads, "the sweeps after online_finish uploaded the sequence again"
    monkeypatch.setattr(SweepEngine, "upload", real_upload)
    # offline: the same messages collected, then the whole pass
    lidar, odo = Lidar(config=cfg), Odometria(config=cfg)
    replay(obs, od, ve, lidar.callback, odo.callback)
    b = ICM_ROS(cfg)
    b.load_messages(lidar, odo)
    b.inicializar_offline()
    for name in names:
        assert np.array_equal(init_a[name], getattr(b, name)), name
    assert np.array_equal(init_a["cant_obs_i"], b.mapa_obj.cant_obs_i)
    assert init_a["lact"] == b.mapa_obj.landmarks_actuales
    mv, x = b.mapa_viejo.copy(), b.positions.copy()
    for k in range(2):
        mv, x = b.iterations_process_offline(mv, x)
        assert np.array_equal(res_a[k][0], mv) and np.array_equal(res_a[k][1], x)
