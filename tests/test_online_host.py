"""ICM_ROS.principal_callback without a GPU: scans and odometry paired by sequence number as their messages arrive,
complete samples queued in seq order, late samples dropped and counted (reference scripts/ICM_SLAM.py:301-341)."""
import numpy as np

from util import gold


def _icm():
    from ICM_ROS import ICM_ROS
    from ICM_SLAM_tools import ConfigICM
    return ICM_ROS(ConfigICM("config_default.yaml"))


def _messages(T=40):
    from matlab2ros.replay import messages
    d = gold("data_IJAC2018.npz")
    return list(messages(d["observations"][:, :T], d["odometry"][:, :T], d["velocities"][:, :T]))


def _queued_seqs(a):
    return [e[0] for e in a._queue]


def test_in_order_replay_queues_what_load_messages_builds():
    from matlab2ros.replay import replay
    from sensors_definitions import Lidar, Odometria
    d = gold("data_IJAC2018.npz")
    T = 60
    a = _icm()
    n = replay(d["observations"][:, :T], d["odometry"][:, :T], d["velocities"][:, :T], a.lidar.callback, a.odom.callback)
    assert n == T and a.dropped_samples == 0 and a.new_data == T
    z, o, u = a.queued_samples()
    b = _icm()
    lidar, odo = Lidar(config=b.config), Odometria(config=b.config)
    replay(d["observations"][:, :T], d["odometry"][:, :T], d["velocities"][:, :T], lidar.callback, odo.callback)
    zb, ob, ub = b.load_messages(lidar, odo)
    assert np.array_equal(z, zb) and np.array_equal(o, ob) and np.array_equal(u, ub)


def test_interleaved_and_one_sided_messages():
    msgs = _messages(8)
    a = _icm()
    # scans 0..3 first, then odometry 0..3 in reverse: nothing completes until a partner arrives
    for s, _ in msgs[:4]:
        a.lidar.callback(s)
    assert _queued_seqs(a) == []
    a.odom.callback(msgs[0][1])
    assert _queued_seqs(a) == [0]
    for _, o in msgs[1:4]:
        a.odom.callback(o)
    assert _queued_seqs(a) == [0, 1, 2, 3]
    # odometry of 4 and 5, scan of 5 only (4 stays one-sided), then 6 with the scan first
    a.odom.callback(msgs[4][1])
    a.odom.callback(msgs[5][1])
    a.lidar.callback(msgs[5][0])
    a.lidar.callback(msgs[6][0])
    a.odom.callback(msgs[6][1])
    assert _queued_seqs(a) == [0, 1, 2, 3, 5, 6] and a.dropped_samples == 0
    # the scan of 4 arrives after 5 was queued: too late, dropped and counted
    a.lidar.callback(msgs[4][0])
    assert _queued_seqs(a) == [0, 1, 2, 3, 5, 6] and a.dropped_samples == 1
    a.odom.callback(msgs[7][1])
    a.lidar.callback(msgs[7][0])
    assert _queued_seqs(a) == [0, 1, 2, 3, 5, 6, 7]
    z, o, u = a.queued_samples()
    assert z.shape == (180, 7) and o.shape == (3, 7) and u.shape == (2, 7)


def test_out_of_order_samples_are_dropped_and_counted():
    msgs = _messages(6)
    a = _icm()
    for k in (0, 2, 1, 3, 5, 4):
        a.odom.callback(msgs[k][1])
        a.lidar.callback(msgs[k][0])
    assert _queued_seqs(a) == [0, 2, 3, 5] and a.dropped_samples == 2
    assert a.online_step.__doc__ and a.icm_iterations_service({}, {}) is True and a.iterations_flag
