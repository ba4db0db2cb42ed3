"""Many independent sequences at once: the initialisation pass and the reference-order sweep of M engines, each with
its own sequence and config, advanced together by one launch per chain form (icm_init_pass_batch, icm_sweep_batch).

Every member gets exactly the bits its own single call gives it.  A malformed batch (no engine, the same engine twice,
engines on different devices, a member without a sequence or state, a sharded member, a cross-check energy form, debug
or optimistic mode, a red-black schedule) raises at once -- ValueError or NotImplementedError, as the single calls do --
and changes nothing.  A data error fails its member only: its slot of the returned list holds the exception its single
call would have raised (IndexError for a new landmark that does not fit in L), and the other members go on.
"""
import ctypes as C
from copy import deepcopy as copy

import numpy as np

from . import _lib
from ._lib import SCHEDULES, dptr
from .engine import _f64, _raise, seed_first_scan


def _exception(rc, msg):
    """The exception instance the single call raises for code rc."""
    try:
        _raise(rc, msg)
    except Exception as e:   # noqa: BLE001  (whatever _raise maps the code to)
        return e
    return None


def _handles(engines):
    engines = list(engines)
    if not engines:
        raise ValueError("a batch needs at least one engine")
    if len({id(e) for e in engines}) != len(engines):
        raise ValueError("the same engine twice in one batch")
    if any(getattr(e, "h", None) is None for e in engines):
        raise ValueError("a closed engine in the batch")
    return engines, (C.c_void_p * len(engines))(*[e.h.value for e in engines])


def _results(lib, engines, rcs):
    """Per member None or its exception (the codes of a batch that ran)."""
    out = []
    for e, r in zip(engines, rcs):
        e.last_rc = int(r)
        out.append(None if r == 0 else _exception(int(r), lib.icm_last_error(e.h).decode()))
    return out


def init_pass_batch(engines, x0s):
    """engines[i].init_pass(x0s[i]) for every i, the causal passes in one launch.  Item i of the returned list is what
    that call returns -- (x_init (3,T), y_raw (2,L), counts (L), landmarks_actuales, scan-0 labels) -- or the exception
    it would raise."""
    engines, _ = _handles(engines)
    x0s = list(x0s)
    if len(x0s) != len(engines):
        raise ValueError("init_pass_batch: one x0 per engine")
    lib = _lib.load()
    res = [None] * len(engines)
    go = []
    state = []
    for i, e in enumerate(engines):
        x0 = _f64(np.asarray(x0s[i], dtype=np.float64).reshape(3))
        try:   # the host part of SweepEngine.init_pass: scan 0 clustered into the first landmarks
            off, bk, d, bx, by = e.kept_beams()
            n0 = int(off[1] - off[0])
            y, cnt, lact, c = seed_first_scan(e.config, x0, bx[:n0], by[:n0])
        except Exception as ex:   # noqa: BLE001  (the member's own exception, as its single call raises it)
            res[i] = ex
            continue
        go.append(i)
        state.append((x0, y, cnt, lact, c, np.zeros((3, e.T))))
    if not go:
        return res
    m = len(go)
    sub = [engines[i] for i in go]
    hsub = (C.c_void_p * m)(*[e.h.value for e in sub])
    pp = C.POINTER(C.c_double)
    x0p = (pp * m)(*[dptr(s[0]) for s in state])
    yp = (pp * m)(*[dptr(s[1]) for s in state])
    cp = (pp * m)(*[dptr(s[2]) for s in state])
    xp = (pp * m)(*[dptr(s[5]) for s in state])
    la = (C.c_int64 * m)(*[int(s[3]) for s in state])
    rcs = (C.c_int32 * m)(*([1] * m))
    rc = lib.icm_init_pass_batch(hsub, m, x0p, yp, cp, la, xp, rcs)
    if rc and all(r == 1 for r in rcs):   # refused as a whole: nothing ran
        _raise(rc, lib.icm_last_error(sub[0].h).decode())
    errs = _results(lib, sub, list(rcs))
    for k, i in enumerate(go):
        x0, y, cnt, _, c, x = state[k]
        res[i] = errs[k] if errs[k] is not None else (x, y, cnt, int(la[k]), c)
    return res


def sweep_batch(engines, schedule="sequential"):
    """engines[i].sweep_device(schedule) for every i, the chains in one launch per energy form (folded / complete).
    Returns a list of None (success) or the exception member i's single call would have raised."""
    engines, hs = _handles(engines)
    if schedule not in SCHEDULES:
        raise ValueError("unknown schedule %r" % (schedule,))
    lib = _lib.load()
    m = len(engines)
    rcs = (C.c_int32 * m)(*([1] * m))
    rc = lib.icm_sweep_batch(hs, m, SCHEDULES[schedule], rcs)
    if rc and all(r == 1 for r in rcs):   # refused as a whole: nothing ran
        _raise(rc, lib.icm_last_error(engines[0].h).decode())
    return _results(lib, engines, list(rcs))


def run_offline(problems, sweeps=None, device=0):
    """A parameter study in one call.  problems: list of (config, mediciones (B,T), odometria (3,T), u (2,T)), the
    arrays as ICM_ROS holds them after load_data.  Per member: ICM_ROS.inicializar_offline() (the causal pass, batched,
    then Mapa.filtrar), then `sweeps` reference-order sweeps (default: config.N of the first member), batched.  Returns
    per member (mapa (2,K), x (3,T)) as the reference's driver loop leaves them (inicializar_offline, then
    `mapa_refinado, x = iterations_process_offline(mapa_viejo, x)` N times), or the member's exception."""
    from ICM_SLAM_tools import Mapa
    from .engine import SweepEngine
    problems = list(problems)
    if not problems:
        raise ValueError("run_offline: no problem")
    if sweeps is None:
        sweeps = int(problems[0][0].N)
    engines, res, x0s = [], [None] * len(problems), []
    try:
        for i, (cfg, med, odo, u) in enumerate(problems):
            e = SweepEngine(cfg, device)
            engines.append(e)
            odo = np.asarray(odo, dtype=np.float64)
            x0s.append(np.array([odo[:, 0]]).T)
            try:
                e.upload(med, odo, u)
            except (ValueError, IndexError, NotImplementedError) as ex:
                res[i] = ex
        live = [i for i in range(len(problems)) if res[i] is None]
        init = init_pass_batch([engines[i] for i in live], [x0s[i] for i in live]) if live else []
        state = {}
        for i, r in zip(live, init):
            if isinstance(r, Exception):
                res[i] = r
                continue
            x, y, cnt, lact, _ = r
            try:   # inicializar_offline: Mapa.filtrar of the raw map
                mo = Mapa(problems[i][0])
                mo.landmarks_actuales = lact
                mo.cant_obs_i = cnt
                yy = mo.filtrar(y)
                yy = yy[:, :mo.landmarks_actuales]
                mapa, x = copy(yy), copy(x)
                engines[i].set_state(mapa, x, x0s[i], mo.landmarks_actuales)
            except Exception as ex:   # noqa: BLE001
                res[i] = ex
                continue
            state[i] = (mapa, x)
        for _ in range(sweeps):
            live = [i for i in sorted(state) if res[i] is None]
            if not live:
                break
            for i, r in zip(live, sweep_batch([engines[i] for i in live], "sequential")):
                if r is not None:
                    res[i] = r
        for i in sorted(state):
            if res[i] is not None:
                continue
            x, mo, _, K = engines[i].get_state()
            res[i] = (mo[:, :K].copy(), x) if sweeps > 0 else state[i]
    finally:
        for e in engines:
            e.close()
    return res
