"""Test-side reference of joint position limits (include/cfs_hip.h, cfs_problem_set_joint_limits), built on
the oracle's own primitives.  The limited get_con is the oracle's dense get_con (Lib/CFS_FANUC.m:101-135) followed by the position
rows of every waypoint i and joint c: +Bpos row (i, c) <= hi_c - theta0_c - (i+1) dt v0_c, then -Bpos row (i, c) <= theta0_c +
(i+1) dt v0_c - lo_c, with Bpos the position rows of Baug.  The outer loop is orc_optimizer (oracle/cfs_oracle.c) restated in
Python, as tests/moving_reference.py does: the QP through O.qp_solve (rows with an infinite bound are left out: they can never be
active), the rollout through O.rollout, the costs through orc_get_cost, the stop tests of Lib/EVAL.m:61-73 and
Lib/PSGCFS_FANUC.m:136-142, one noise row per PSG step.  Used by tests/test_limits_reference.py (which validates it against
O.optimizer) and tests/test_gpu_limits.py (which checks the device against it)."""
from types import SimpleNamespace

import numpy as np

from moving_reference import _get_cost, obs_cell


def pos_rows(s, xR1, limits):
    """(A (2nn, nn), b (2nn,)): the position rows [+pos (i, c) | -pos (i, c)] of a limited handle.  limits: (nj, 2) [lo, hi]."""
    H, nj, ns, dt = s.H, s.njoint, 2 * s.njoint, s.robot.delta_t
    lim = np.asarray(limits, float)
    Baug = np.asarray(s.Baug, float)
    Bpos = np.stack([Baug[i * ns + c] for i in range(H) for c in range(nj)])
    xR1 = np.asarray(xR1, float)
    pos = np.array([xR1[c] + ((i + 1) * dt) * xR1[nj + c] for i in range(H) for c in range(nj)])
    lo, hi = np.tile(lim[:, 0], H), np.tile(lim[:, 1], H)
    return np.vstack([Bpos, -Bpos]), np.concatenate([hi - pos, pos - lo])


def get_con_limited(O, ROBOT, s, obs, x_, u, mode, limits):
    """(Ainq, binq) of a limited handle: the oracle's rows in its order, then the position rows.  s needs xR1."""
    A, b, *_ = O.get_con(ROBOT, s, obs, x_, u, mode=mode)
    Ap, bp = pos_rows(s, s.xR1, limits)
    return np.vstack([A, Ap]), np.concatenate([b, bp])


def qp_limited(O, G, g0, A, b):
    """O.qp_solve without the rows whose bound is infinite; lambda is returned on every row (0 on the left-out ones)."""
    keep = np.isfinite(b)
    x, lam_k, it, st, kkt = O.qp_solve(G, g0, A[keep], b[keep])
    lam = np.zeros(b.size)
    lam[keep] = lam_k
    return x, lam, it, st, kkt


def optimizer_limited(O, ROBOT, s, obs, mode, limits, x_init=None, xR1=None, ff=None, caug=None, noise=None):
    """CFS_FANUC / PSGCFS_FANUC .optimizer() of one problem with joint position limits (orc_optimizer's loop).  obs: the oracle's
    obs cell; limits: (nj, 2); noise: (rows, nn) or None.  Returns a namespace like O.optimizer's (u, x_, iter_O, total_iter,
    status, cost_all, e_cost_all, e_u_all)."""
    H, nj = s.H, s.njoint
    nn, dt, K = H * nj, s.robot.delta_t, s.MAX_O_ITER
    x_init = s.x_ if x_init is None else x_init
    xR1 = s.xR1 if xR1 is None else xR1
    ff = s.ff if ff is None else ff
    caug = s.caug if caug is None else caug
    s2 = SimpleNamespace(**vars(s))
    s2.xR1, s2.robot = np.asarray(xR1, float), O.robotproperty2(ROBOT)
    QQ, ff = np.asarray(s.QQ, float), np.asarray(ff, float)
    Ap, bp = pos_rows(s2, xR1, limits)
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
        A, b, *_ = O.get_con(ROBOT, s2, obs, x_, u, mode=mode)
        if mode == "CFS":
            A = np.vstack([A, np.eye(nn), -np.eye(nn), Ap])
            b = np.concatenate([b, s.MAX_input, s.MAX_input, bp])
            x, _, it, st, _ = qp_limited(O, QQ, ff, A, b)            # CFS_FANUC.m:85 with the position rows
            total += it
            if st:
                status = st
                break
            u = x
            x_old = x_.copy()                                        # CFS_FANUC.m:88
            x_ = O.rollout(H, nj, dt, xR1, u)
            ev_x = x_.copy()
        else:
            A, b = np.vstack([A, Ap]), np.concatenate([b, bp])
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
                x, _, it, st, _ = qp_limited(O, np.eye(nn), -uu, A, b)   # PSGCFS_FANUC.m:117-120 with the position rows
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


def batch_limited(O, s, bt, mode, idx, limits, x_init=None, workers=16):
    """optimizer_limited for problems idx of a config3 batch (threads: the oracle's C calls release the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    margin = bt.margin_cfs if mode == "CFS" else bt.margin_psg
    xi = bt.x_init if x_init is None else x_init

    def one(b):
        nz = bt.noise[b] if (mode == "PSGCFS" and bt.noise is not None) else None
        return optimizer_limited(O, "M200i", s, obs_cell(bt.obs[b], margin), mode, limits, x_init=xi[b], xR1=bt.xR1[b],
                                 ff=bt.ff[b], caug=bt.caug[b], noise=nz)
    with ThreadPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(one, list(idx)))


def chaotic_limited(O, s, bt, mode, idx, want, limits, kick=1e-12, move=1e-6, seed=1):
    """helpers.chaotic_problems' rule for the limited reference (one kick): problems of idx whose reference answer moves by more
    than `move` rad, or changes status / iteration count, when x_init is perturbed by N(0, kick^2).  Returns (mask, moved_by)."""
    rng = np.random.default_rng(seed)
    xi = bt.x_init + kick * rng.standard_normal(bt.x_init.shape)
    got = batch_limited(O, s, bt, mode, idx, limits, x_init=xi)
    mv = np.array([np.abs(g.x_ - w.x_).max() for g, w in zip(got, want)])
    flip = np.array([(g.status != w.status) or (g.iter_O != w.iter_O) for g, w in zip(got, want)])
    return (mv > move) | flip, mv
