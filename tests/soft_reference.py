"""Test-side reference of the soft-constraint QP (include/cfs_hip.h, CFS_INFEAS_SOFTEN), built on the
oracle's own QP solver: the soft QP is solved as an ordinary QP in the augmented variables (u, s),

    min 1/2 u'Gu + g0'u + mu/2 |s|^2   s.t.   A_col u - s <= b_col,   A_rest u <= b_rest,

so nothing of the device's reduction (1/mu on the Gram diagonal) is assumed.  Used by tests/test_soft_qp_reference.py (which
validates it) and tests/test_gpu_soft.py (which checks the device against it)."""
from types import SimpleNamespace

import numpy as np


def collision_rows(nobs, H, nj):
    """indices of the collision rows in the reference's dense row order (per (j, i): 1 collision, nj +vel, nj -vel)"""
    return np.arange(0, nobs * H * (1 + 2 * nj), 1 + 2 * nj)


def augment(G, g0, A, col, mu):
    """(G_aug, g_aug, A_aug) of the soft QP in (u, s): blkdiag(G, mu I), [g0; 0], [A, -E] with E selecting the collision rows"""
    n, m, nc = G.shape[0], A.shape[0], len(col)
    Ga = np.zeros((n + nc, n + nc))
    Ga[:n, :n] = G
    Ga[n:, n:] = mu * np.eye(nc)
    E = np.zeros((m, nc))
    E[col, np.arange(nc)] = 1.0
    return Ga, np.concatenate([g0, np.zeros(nc)]), np.hstack([A, -E])


def soft_qp(O, G, g0, A, b, col, mu):
    """the soft QP through O.qp_solve on the augmented matrices.  Returns (u, s, lam, status, kkt); lam over the rows of A."""
    n = G.shape[0]
    Ga, ga, Aa = augment(G, g0, A, col, mu)
    x, lam, _, st, kkt = O.qp_solve(Ga, ga, Aa, b)
    return x[:n], x[n:], lam, st, kkt


def least_violation(A, b, col, box=None):
    """phase-1 LP (scipy HiGHS): min t s.t. A_col u - t <= b_col, the other rows hard, |u| <= box, t >= 0 -- the least
    possible max violation of the collision rows (0: the hard QP is feasible)"""
    from scipy.optimize import linprog
    n = A.shape[1]
    iscol = np.zeros(A.shape[0])
    iscol[col] = 1.0
    c = np.zeros(n + 1)
    c[-1] = 1.0
    bounds = [(-m, m) for m in box] if box is not None else [(None, None)] * n
    r = linprog(c, A_ub=np.hstack([A, -iscol[:, None]]), b_ub=b, bounds=bounds + [(0, None)], method="highs")
    assert r.status == 0, r.message
    return float(r.fun)


def step_qp(O, ROBOT, s, obs, xR1, ff, u_prev, k, mode, noise_row=None):
    """the QP of outer iteration k (1-based) from the iterate u_prev (ignored for k = 1: u = 0, x_ = s.x_), exactly as
    Lib/CFS_FANUC.m:66-85 | Lib/PSGCFS_FANUC.m:86-120 pose it.  Returns a namespace (G, g0, A, b, col, box, dist)."""
    H, nj = s.H, s.njoint
    nn = H * nj
    s2 = SimpleNamespace(**vars(s))
    s2.xR1 = xR1
    if k == 1:
        u, x_ = np.zeros(nn), np.asarray(s.x_, float).reshape(-1)
    else:
        u = np.asarray(u_prev, float)
        x_ = O.rollout(H, nj, s.robot.delta_t, xR1, u)
    A, b, dist, _, _ = O.get_con(ROBOT, s2, obs, x_, u, mode=mode)
    col = collision_rows(len(obs), H, nj)
    if mode == "CFS":
        G, g0, box = s.QQ, ff, s.MAX_input
        A = np.vstack([A, np.eye(nn), -np.eye(nn)])
        b = np.concatenate([b, s.MAX_input, s.MAX_input])
    else:
        nz = np.zeros(nn) if noise_row is None else noise_row
        u_ = u - s.alpha * ((s.QQ @ u + ff) + 10.0 * nz / (float(k) * float(k) + 1.0))      # PSGCFS_FANUC.m:109
        G, g0, box = np.eye(nn), -u_, None
    return SimpleNamespace(G=G, g0=g0, A=A, b=b, col=col, box=box, dist=dist)


def oracle_soft_step(O, q, mu):
    """the hard QP when the oracle solves it, otherwise the soft one.  Returns (u, softened, max slack, status, lam)."""
    x, lam, _, st, _ = O.qp_solve(q.G, q.g0, q.A, q.b)
    if st == 0:
        return x, False, 0.0, 0, lam
    u, sl, lam, st, _ = soft_qp(O, q.G, q.g0, q.A, q.b, q.col, mu)
    return u, True, float(sl.max()) if sl.size else 0.0, st, lam
