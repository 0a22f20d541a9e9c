"""Test-side reference of per-waypoint obstacles (include/cfs_hip.h, CFS_OBS_PER_WAYPOINT), built on the
oracle's own primitives.  Collision row (j, i) of get_con (Lib/CFS_FANUC.m:110-120) depends only on waypoint i's pose and on
obstacle j, so the per-waypoint get_con takes, from one oracle get_con per waypoint i (with the obstacles of waypoint i), the rows
of waypoint i.  The outer loop is orc_optimizer (oracle/cfs_oracle.c) restated in Python on top of it: the QP through O.qp_solve,
the rollout through O.rollout, the costs through orc_get_cost, the stop tests of Lib/EVAL.m:61-73 and Lib/PSGCFS_FANUC.m:136-142,
one noise row per PSG step.  Used by tests/test_moving_reference.py (which validates it against O.optimizer) and
tests/test_gpu_moving.py (which checks the device against it)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np


def obs_cell(rows, margin):
    """(nobs, 6) rows -> the oracle's obs cell, margin as both epsilon (CFS) and D (PSGCFS)"""
    return [dict(l=np.stack([np.asarray(r[:3], float), np.asarray(r[3:], float)], axis=1), epsilon=float(m), D=float(m))
            for r, m in zip(rows, margin)]


def get_con_moving(O, ROBOT, s, obs_traj, margin, x_, u, mode):
    """get_con with obstacle rows per waypoint.  obs_traj: (H, nobs, 6); s needs xR1.  Returns (Ainq, binq, dist (nobs, H),
    linkid (nobs, H), grad (nobs, H, nj)) in the reference's row order (rows (j*H + i)*(1+2nj) ... belong to (j, i))."""
    H, nj = s.H, s.njoint
    nobs, per = obs_traj.shape[1], 1 + 2 * nj
    A, b = np.zeros((nobs * H * per, H * nj)), np.zeros(nobs * H * per)
    dist, lid, grad = np.zeros((nobs, H)), np.zeros((nobs, H), np.int32), np.zeros((nobs, H, nj))
    for i in range(H):
        Ai, bi, di, li, gi = O.get_con(ROBOT, s, obs_cell(obs_traj[i], margin), x_, u, mode=mode)
        for j in range(nobs):
            r = slice((j * H + i) * per, (j * H + i + 1) * per)
            A[r], b[r] = Ai[r], bi[r]
        dist[:, i], lid[:, i], grad[:, i] = di[:, i], li[:, i], gi[:, i]
    return A, b, dist, lid, grad


def _get_cost(O, QQ, ff, caug, u):
    fn = O.lib().orc_get_cost
    fn.restype = C.c_double
    QQf = np.asfortranarray(QQ, dtype=np.float64)
    ff, u = np.ascontiguousarray(ff, float), np.ascontiguousarray(u, float)
    return float(fn(C.c_int(u.size), QQf.ctypes.data_as(C.c_void_p), ff.ctypes.data_as(C.c_void_p), C.c_double(caug),
                    u.ctypes.data_as(C.c_void_p)))


def optimizer_moving(O, ROBOT, s, obs_traj, margin, mode, x_init, xR1, ff, caug, noise=None):
    """CFS_FANUC / PSGCFS_FANUC .optimizer() of one problem with obstacle rows per waypoint (orc_optimizer's loop).
    obs_traj: (H, nobs, 6); noise: (rows, nn) or None.  Returns a namespace like O.optimizer's (u, x_, iter_O, total_iter,
    status, cost_all, e_cost_all, e_u_all)."""
    H, nj = s.H, s.njoint
    nn, dt, K = H * nj, s.robot.delta_t, s.MAX_O_ITER
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
        A, b, *_ = get_con_moving(O, ROBOT, s2, obs_traj, margin, x_, u, mode)
        if mode == "CFS":
            A = np.vstack([A, np.eye(nn), -np.eye(nn)])
            b = np.concatenate([b, s.MAX_input, s.MAX_input])
            x, _, it, st, _ = O.qp_solve(QQ, ff, A, b)              # CFS_FANUC.m:85
            total += it
            if st:
                status = st
                break
            u = x
            x_old = x_.copy()                                        # CFS_FANUC.m:88
            x_ = O.rollout(H, nj, dt, xR1, u)
            ev_x = x_.copy()
        else:
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
                x, _, it, st, _ = O.qp_solve(np.eye(nn), -uu, A, b)  # PSGCFS_FANUC.m:117-120
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


def batch_moving(O, s, bt, mode, idx, x_init=None, workers=16):
    """optimizer_moving for problems idx of a config3_moving batch (threads: the oracle's C calls release the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    margin = bt.margin_cfs if mode == "CFS" else bt.margin_psg
    xi = bt.x_init if x_init is None else x_init

    def one(b):
        nz = bt.noise[b] if (mode == "PSGCFS" and bt.noise is not None) else None
        return optimizer_moving(O, "M200i", s, bt.obs[b], margin, mode, xi[b], bt.xR1[b], bt.ff[b], bt.caug[b], noise=nz)
    with ThreadPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(one, list(idx)))


def chaotic_moving(O, s, bt, mode, idx, want, kick=1e-12, move=1e-6, seed=1):
    """helpers.chaotic_problems' rule for the moving reference (one kick): problems of idx whose reference answer moves by more
    than `move` rad, or changes status / iteration count, when x_init is perturbed by N(0, kick^2).  Returns (mask, moved_by)."""
    rng = np.random.default_rng(seed)
    xi = bt.x_init + kick * rng.standard_normal(bt.x_init.shape)
    got = batch_moving(O, s, bt, mode, idx, x_init=xi)
    mv = np.array([np.abs(g.x_ - w.x_).max() for g, w in zip(got, want)])
    flip = np.array([(g.status != w.status) or (g.iter_O != w.iter_O) for g, w in zip(got, want)])
    return (mv > move) | flip, mv
