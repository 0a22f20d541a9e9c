"""The one test-side restatement of the CFS_FANUC / PSGCFS_FANUC .optimizer() loop (orc_optimizer, oracle/cfs_oracle.c), built on
the oracle's own primitives: the QP through O.qp_solve (or the caller's wrapper of it), the rollout through O.rollout, the costs
through orc_get_cost, the stop tests of Lib/EVAL.m:61-73 and Lib/PSGCFS_FANUC.m:136-142, one noise row per PSG step.  A feature's
reference (tests/moving_reference.py, tests/limits_reference.py, tests/mesh_motion_reference.py) supplies what it changes as
arguments: its get_con, rows appended to every QP, a QP wrapper.  Nothing here is looked up in another module at call time, so
any number of these loops may run on threads of one process.  Also the thread-pool fan-out and the one-kick chaos rule that the
references share."""
import ctypes as C
from types import SimpleNamespace

import numpy as np


def _get_cost(O, QQ, ff, caug, u):
    fn = O.lib().orc_get_cost
    fn.restype = C.c_double
    QQf = np.asfortranarray(QQ, dtype=np.float64)
    ff, u = np.ascontiguousarray(ff, float), np.ascontiguousarray(u, float)
    return float(fn(C.c_int(u.size), QQf.ctypes.data_as(C.c_void_p), ff.ctypes.data_as(C.c_void_p), C.c_double(caug),
                    u.ctypes.data_as(C.c_void_p)))


def optimizer(O, ROBOT, s, mode, get_con, x_init, xR1, ff, caug, noise=None, extra_rows=None, qp=None):
    """CFS_FANUC / PSGCFS_FANUC .optimizer() of one problem (orc_optimizer's loop).  get_con(s2, x_, u) -> (A, b, ...) gives the
    collision rows, s2 being s with xR1 and the oracle's robot; extra_rows: an (A, b) appended after the input-bound rows (CFS) or
    after the collision rows (PSGCFS), or None; qp: O.qp_solve's signature (default O.qp_solve); noise: (rows, nn) or None.
    Returns a namespace like O.optimizer's (u, x_, iter_O, total_iter, status, cost_all, e_cost_all, e_u_all)."""
    H, nj = s.H, s.njoint
    nn, dt, K = H * nj, s.robot.delta_t, s.MAX_O_ITER
    qp = O.qp_solve if qp is None else qp
    s2 = SimpleNamespace(**vars(s))
    s2.xR1, s2.robot = np.asarray(xR1, float), O.robotproperty2(ROBOT)
    QQ, ff = np.asarray(s.QQ, float), np.asarray(ff, float)
    x_ = np.asarray(x_init, float).copy()
    u = np.zeros(nn)
    ev_x, x_old = x_.copy(), np.ones_like(x_)                      # EVAL.m:46-47
    cost_old, cost_new = 100000.0, _get_cost(O, QQ, ff, caug, u)   # EVAL.m:29
    iter_O, total, noise_row, status = 1, 0, 0, 1
    cost_all, e_cost_all, e_u_all = [], [], []
    while True:
        if np.linalg.norm(ev_x - x_old) < s.epsilon_O:              # EVAL.m:61-73
            status = 0
            break
        if iter_O > K:
            status = 1
            break
        u_old = u.copy()
        if mode == "CFS":
            cost_old = cost_new                                      # CFS_FANUC.m:67
        A, b, *_ = get_con(s2, x_, u)
        if mode == "CFS":
            A = np.vstack([A, np.eye(nn), -np.eye(nn)])
            b = np.concatenate([b, s.MAX_input, s.MAX_input])
            if extra_rows is not None:
                A, b = np.vstack([A, extra_rows[0]]), np.concatenate([b, extra_rows[1]])
            x, _, it, st, _ = qp(QQ, ff, A, b)                      # CFS_FANUC.m:85
            total += it
            if st:
                status = st
                break
            u = x
            x_old = x_.copy()                                        # CFS_FANUC.m:88
            x_ = O.rollout(H, nj, dt, xR1, u)
            ev_x = x_.copy()
        else:
            if extra_rows is not None:
                A, b = np.vstack([A, extra_rows[0]]), np.concatenate([b, extra_rows[1]])
            iter_I, rc = 1, 0                                        # inner_PSG_5, MAX_I_ITER = 1 (PSGCFS_FANUC.m:86-103, 136-142)
            while not (abs(cost_new - cost_old) < 1e-4 or iter_I > 1):
                cost_old = cost_new
                sc = float(iter_O) * float(iter_O) + 1.0
                nz = noise[noise_row] if (noise is not None and noise_row < len(noise)) else np.zeros(nn)
                gq = np.zeros(nn)
                for c in range(nn):                                  # QQ*u summed in the oracle's order
                    gq += QQ[:, c] * u[c]
                uu = u - s.alpha * ((gq + ff) + 10.0 * nz / sc)      # PSGCFS_FANUC.m:109
                noise_row += 1
                x, _, it, st, _ = qp(np.eye(nn), -uu, A, b)         # PSGCFS_FANUC.m:117-120
                total += it
                if st:
                    rc = st
                    break
                u = x
                cost_new = _get_cost(O, QQ, ff, caug, u)
                iter_I += 1
            if rc:
                status = rc
                break
            x_ = O.rollout(H, nj, dt, xR1, u)
            ev_x = x_.copy()                                         # x_old is never refreshed
        cost_new = _get_cost(O, QQ, ff, caug, u)
        cost_all.append(cost_new)                                    # store_result (EVAL.m:55-59)
        e_cost_all.append(abs(cost_old - cost_new))
        e_u_all.append(float(np.linalg.norm(u_old - u)))
        iter_O += 1
    return SimpleNamespace(u=u, x_=x_, iter_O=iter_O, total_iter=total, status=status, cost_all=np.array(cost_all),
                           e_cost_all=np.array(e_cost_all), e_u_all=np.array(e_u_all))


def batch(one_problem, idx, workers=16):
    """[one_problem(b) for b in idx] on threads: the oracle's C calls release the GIL"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(one_problem, list(idx)))


def chaotic(batch_fn, bt, idx, want, kick=1e-12, move=1e-6, seed=1):
    """helpers.chaotic_problems' rule with one kick: problems of idx whose reference answer batch_fn(idx, x_init) moves by more
    than `move` rad, or changes status / iteration count, when x_init is perturbed by N(0, kick^2).  Returns (mask, moved_by)."""
    rng = np.random.default_rng(seed)
    xi = bt.x_init + kick * rng.standard_normal(bt.x_init.shape)
    got = batch_fn(idx, xi)
    mv = np.array([np.abs(g.x_ - w.x_).max() for g, w in zip(got, want)])
    flip = np.array([(g.status != w.status) or (g.iter_O != w.iter_O) for g, w in zip(got, want)])
    return (mv > move) | flip, mv
