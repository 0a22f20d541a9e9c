"""Test-side reference of the clearance audit (include/cfs_hip.h, cfs_clearance): NumPy over the oracle's
dist_arm.  The contract is restated literally -- H intervals of S+1 samples each, sample k of interval i at tau = k*delta_t/S on
the double integrator theta_s + tau*v_s + tau^2/2*u_i (robotproperty2.m:136-139), sample S at row i of x_ itself -- without the
device's shortcuts (it does not merge sample S of one interval with sample 0 of the next).  Used by
tests/test_clearance_reference.py (which checks the bound against a 16x denser sampling) and tests/test_gpu_clearance.py (which
checks the device against it)."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np


def rho_matrix(robot, nj):
    """rho[m, k], m <= k: no point of capsule k is farther than this from the axis of joint m: the link translations between them
    (hypot(a_j, d_j) of DH row j; 2L: |robot.T(:, j+1)|, the translation link j applies) plus the farther end of capsule k"""
    rho = np.zeros((nj, nj))
    for k in range(nj):
        ck = float(np.sqrt((np.asarray(robot.cap[k], float) ** 2).sum(axis=0)).max())
        ln = 0.0
        for m in range(k, -1, -1):
            ln += float(np.sqrt((robot.T[:, m + 1] ** 2).sum())) if robot.name == "2L" else math.hypot(robot.DH[m, 2], robot.DH[m, 1])
            rho[m, k] = ln + ck
    return rho


def _dist_all(O, robot, TH, OB):
    """oracle dist_arm of N poses TH (N, nj) against their own obstacle rows OB (N, nobs, 6): d (N, nobs), linkid (N, nobs).
    O.dist_arm's C function, called with one robot struct for all poses."""
    fn, rb = O.lib().orc_dist_arm, O.c_robot(robot)
    TH, OB = np.ascontiguousarray(TH, float), np.ascontiguousarray(OB, float)
    N, nj = TH.shape
    nobs = OB.shape[1]
    d, lk = np.empty((N, nobs)), np.empty((N, nobs), np.int32)
    lid, rbp, cnj = C.c_int(0), C.byref(rb), C.c_int(nj)
    lidp = C.byref(lid)
    pt, po = TH.ctypes.data, OB.ctypes.data
    for n in range(N):
        tp = C.c_void_p(pt + n * nj * 8)
        for j in range(nobs):
            d[n, j] = fn(rbp, tp, cnj, C.c_void_p(po + (n * nobs + j) * 48), lidp)
            lk[n, j] = lid.value
    return d, lk


def samples(H, nj, dt, x_, u, xR1, obs, S):
    """poses (H, S+1, nj) and obstacle rows (H, S+1, nobs, 6) of every sample of the contract; obs (nobs, 6) or (H, nobs, 6)"""
    X, U, xR1 = np.asarray(x_, float).reshape(H, 2 * nj), np.asarray(u, float).reshape(H, nj), np.asarray(xR1, float)
    obs = np.asarray(obs, float)
    nobs = obs.shape[-2]
    TH, OB = np.empty((H, S + 1, nj)), np.empty((H, S + 1, nobs, 6))
    for i in range(H):
        s = xR1 if i == 0 else X[i - 1]
        for k in range(S + 1):
            tau = k * dt / S
            TH[i, k] = X[i, :nj] if k == S else s[:nj] + tau * s[nj:] + tau * tau / 2 * U[i]
            if obs.ndim == 2:
                OB[i, k] = obs
            elif i == 0 or k == S:
                OB[i, k] = obs[i]                     # held at row 0 in interval 0; the waypoint's own row at k = S
            else:
                OB[i, k] = obs[i - 1] + (k / S) * (obs[i] - obs[i - 1])
    return TH, OB


def audit(O, robot, H, nj, dt, x_, u, xR1, obs, S):
    """cfs_clearance of one problem.  Returns a namespace of (nobs,) arrays: dist_wp, dist_path, dist_lower, t_path, link_path, and
    for the tests gap (how far above the minimum the lowest sample at ANOTHER time is: sample S of interval i and sample 0 of
    interval i+1 are the same instant and the same number), L_max (the largest L of any sub-interval) and D (H, S+1, nobs)."""
    X, U, xR1 = np.asarray(x_, float).reshape(H, 2 * nj), np.asarray(u, float).reshape(H, nj), np.asarray(xR1, float)
    obs = np.asarray(obs, float)
    nobs = obs.shape[-2]
    TH, OB = samples(H, nj, dt, x_, u, xR1, obs, S)
    d, lk = _dist_all(O, robot, TH.reshape(-1, nj), OB.reshape(-1, nobs, 6))
    D, LK = d.reshape(H, S + 1, nobs), lk.reshape(H, S + 1, nobs)
    rho = rho_matrix(robot, nj)
    L = np.zeros((H, S, nobs))
    for i in range(H):
        v0 = xR1[nj:] if i == 0 else X[i - 1, nj:]
        vo = np.zeros(nobs)
        if obs.ndim == 3 and i > 0:
            mv = obs[i] - obs[i - 1]
            vo = np.maximum(np.sqrt((mv[:, :3] ** 2).sum(axis=1)), np.sqrt((mv[:, 3:] ** 2).sum(axis=1))) / dt
        for k in range(S):
            w = np.maximum(np.abs(v0 + (k * dt / S) * U[i]), np.abs(v0 + ((k + 1) * dt / S) * U[i]))
            L[i, k] = max(float(w[:kk + 1] @ rho[:kk + 1, kk]) for kk in range(nj)) + vo
    low = (D[:, :-1] + D[:, 1:]) / 2 - L * dt / (2 * S)
    flat = D.reshape(-1, nobs)
    first = flat.argmin(axis=0)                       # first minimum: lowest interval, then lowest k
    i_min, k_min = first // (S + 1), first % (S + 1)
    t_all = ((np.arange(H)[:, None] + np.arange(S + 1)[None, :] / S) * dt).reshape(-1)
    t_path = (i_min + k_min / S) * dt
    gap = np.array([(flat[t_all != t_path[j], j].min() - flat[first[j], j]) for j in range(nobs)])
    return SimpleNamespace(dist_wp=D[:, S].min(axis=0), dist_path=flat.min(axis=0), dist_lower=low.reshape(-1, nobs).min(axis=0),
                           t_path=t_path, link_path=LK.reshape(-1, nobs)[first, np.arange(nobs)], gap=gap,
                           L_max=L.reshape(-1, nobs).max(axis=0), D=D)


def audit_batch(O, robot, H, nj, dt, x_, u, xR1, obs, S, idx=None):
    """audit() of problems idx (default: all) of a batch; every field stacked along a leading axis (D left out)"""
    idx = range(len(x_)) if idx is None else idx
    rs = [audit(O, robot, H, nj, dt, x_[b], u[b], xR1[b], obs[b], S) for b in idx]
    return SimpleNamespace(**{k: np.stack([getattr(r, k) for r in rs]) for k in ("dist_wp", "dist_path", "dist_lower", "t_path", "link_path", "gap", "L_max")})


def dense_min(O, robot, H, nj, dt, x_, u, xR1, obs, S):
    """min of dist_arm over the S-sample grid, (nobs,): the stand-in for continuous time in the soundness test"""
    nobs = np.asarray(obs).shape[-2]
    TH, OB = samples(H, nj, dt, x_, u, xR1, obs, S)
    return _dist_all(O, robot, TH.reshape(-1, nj), OB.reshape(-1, nobs, 6))[0].min(axis=0)
