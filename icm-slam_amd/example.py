"""Counterpart of the reference's `scripts/example.py`: the same driver loop
(scripts/example.py:37-54), offline.  The reference needs a live rosbridge; here the recorded
sequence named by `config.file` is loaded and `inicializar_offline()` runs the same
initialisation pass on it.

    python example.py [--online] [config.yaml] [data.mat|data.npz]

--online: the reference's online front door instead (scripts/ICM_ROS.py:57-119): every sample of the data file is
replayed as a LaserScan / Odometry message pair (matlab2ros.replay) into ICM.lidar / ICM.odom, and online_step()
advances the initialisation pass as the samples arrive; online_finish() then hands over to the usual sweeps.
"""
import sys
from copy import deepcopy as copy

import numpy as np

from ICM_ROS import ICM_ROS
from ICM_SLAM_tools import ConfigICM, calc_cambio


class My_method(ICM_ROS):
    """Placeholders of the reference's example subclass (scripts/example.py:13-35): methods with a
    trailing underscore are never called.  Overriding g/h/fun_x/fun_xn themselves is refused by
    the HIP build (Python callbacks cannot run inside the kernels)."""

    def __init__(self, config):
        ICM_ROS.__init__(self, config)


def inicializar_por_mensajes(ICM, file=None):
    """Replay the data file's samples as messages into the subscribers, one online_step per sample."""
    from matlab2ros.replay import replay
    z, odo, vel = ICM.read_data_file(file)

    def on_scan(msg):
        ICM.lidar.callback(msg)
        ICM.online_step()

    replay(z, odo, vel, on_scan, ICM.odom.callback)
    ICM.online_step()
    ICM.online_finish()
    print('online: %d samples, %d dropped, %d landmarks' % (ICM.positions.shape[1], ICM.dropped_samples, ICM.mapa_viejo.shape[1]))


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if a != '--online']
    online = len(args) != len(sys.argv) - 1
    config = ConfigICM(args[0] if args else 'config_default.yaml')
    ICM = ICM_ROS(config)
    if online:
        inicializar_por_mensajes(ICM, args[1] if len(args) > 1 else None)
    else:
        ICM.load_data(args[1] if len(args) > 1 else None)
        ICM.inicializar_offline()
    if ICM.iterations_flag:
        mapa_viejo = copy(ICM.mapa_viejo)
        x = copy(ICM.positions)
        for iteracionICM in range(config.N):
            print('iteración ICM : ', iteracionICM + 1)
            mapa_refinado, x = ICM.iterations_process_offline(mapa_viejo, x)
            print('Correccion: ', np.linalg.norm(x - ICM.positions, axis=1).sum(),
                  ' cambio (min,max,medio): ', calc_cambio(mapa_refinado, mapa_viejo))
            mapa_viejo = copy(mapa_refinado)  # as scripts/ICM_ROS.py:311
