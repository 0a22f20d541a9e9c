"""Test-side reference of the clearance audit with moving meshes (include/cfs_hip.h, cfs_clearance_mesh_motion; DESIGN.md section
26): the contract restated in NumPy over the oracle.  Every one of the H*(S+1) samples of tests/clearance_reference.py registers
mesh j's triangles where that sample's FORWARD pose puts them (no inverse pose, no hierarchy, no merged samples) and takes the
oracle's dist_arm; the bound adds the mesh's surface speed to the arm's share of L.  The oracle's mesh registry is global, so this
runs sequentially.  Used by tests/test_clearance_motion_reference.py (which checks the helper and the bound) and
tests/test_gpu_clearance_motion.py (which checks the device against it)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

import clearance_reference as CR
from mesh_motion_reference import FIRST_ID, transform

QUARTER_TURN = "quarter turn"


def mesh_frame(tri):
    """(c, r): the centre (min + max) / 2 of the bounding box of the vertices, and the largest distance of a vertex from it"""
    V = np.asarray(tri, float).reshape(-1, 3)
    c = (V.min(axis=0) + V.max(axis=0)) / 2
    return c, float(np.sqrt(((V - c) ** 2).sum(axis=1)).max())


def rodrigues(a, ang):
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(ang) * K + (1.0 - np.cos(ang)) * (K @ K)


def interval(T0, T1, c, r, dt):
    """the motion of a mesh with frame (c, r) from pose T0 (tau = 0) to pose T1 (tau = delta_t): held (the two poses are bitwise
    equal: the mesh stands at T1), else axis a, angle theta, R0, the centre's two positions c0 / c1, and in both cases v, the bound
    of the speed of every surface point"""
    T0, T1 = np.asarray(T0, float)[:3], np.asarray(T1, float)[:3]
    if T0.tobytes() == T1.tobytes():
        return SimpleNamespace(held=True, T=T1, v=0.0, theta=0.0)
    R0, R1 = T0[:, :3], T1[:, :3]
    Rr = R1 @ R0.T
    if np.trace(Rr) < 1.0:
        raise ValueError(QUARTER_TURN)
    w = np.array([Rr[2, 1] - Rr[1, 2], Rr[0, 2] - Rr[2, 0], Rr[1, 0] - Rr[0, 1]]) / 2
    nw = float(np.sqrt((w ** 2).sum()))
    theta = float(np.arctan2(nw, (np.trace(Rr) - 1.0) / 2))
    a = w / nw if nw > 0.0 else np.zeros(3)
    c0, c1 = R0 @ c + T0[:, 3], R1 @ c + T1[:, 3]
    return SimpleNamespace(held=False, T=T1, a=a, theta=theta, R0=R0, c=c, c0=c0, c1=c1,
                           v=(theta * r + float(np.sqrt(((c1 - c0) ** 2).sum()))) / dt)


def rotation_at(itv, s):
    return rodrigues(itv.a, s * itv.theta) @ itv.R0


def pose_at(itv, s, stored=False):
    """3x4 forward pose of the mesh at s in [0, 1] of the interval; stored: the interval's own waypoint pose, unchanged (what a
    sample at k = S, a held interval and interval 0 use)"""
    if stored or itv.held:
        return itv.T
    R = rotation_at(itv, s)
    cw = itv.c0 + s * (itv.c1 - itv.c0)
    return np.concatenate([R, (cw - R @ itv.c)[:, None]], axis=1)


def intervals(tri, poses, dt):
    """the H intervals of one mesh: interval 0 holds pose 0"""
    c, r = mesh_frame(tri)
    P = np.asarray(poses, float)
    return [interval(P[max(i - 1, 0)], P[i], c, r, dt) for i in range(len(P))]


def sample_pose(itvs, i, k, S):
    return pose_at(itvs[i], k / S, stored=(i == 0 or k == S))


def _distances(O, robot, TH, lines, tris, itvs, S):
    """D, LK (H, S+1, nobs): oracle dist_arm of every sample against the lines and against every mesh where the sample's pose puts it"""
    H, _, nj = TH.shape
    nline, nobs = len(lines), len(lines) + len(tris)
    fn, rb = O.lib().orc_dist_arm, O.c_robot(robot)
    lid = C.c_int(0)
    D, LK = np.empty((H, S + 1, nobs)), np.empty((H, S + 1, nobs), np.int32)
    rows = np.ascontiguousarray(np.asarray(lines, float).reshape(nline, 6))
    for i in range(H):
        for k in range(S + 1):
            th = np.ascontiguousarray(TH[i, k])
            for j in range(nobs):
                if j < nline:
                    row = rows[j]
                else:
                    jm = j - nline
                    l = O.mesh_register(FIRST_ID + jm, transform(tris[jm], sample_pose(itvs[jm], i, k, S)))
                    row = np.ascontiguousarray(np.concatenate([l[:, 0], l[:, 1]]))
                D[i, k, j] = fn(C.byref(rb), C.c_void_p(th.ctypes.data), C.c_int(nj), C.c_void_p(row.ctypes.data), C.byref(lid))
                LK[i, k, j] = lid.value
    return D, LK


def audit(O, robot, H, nj, dt, x_, u, xR1, lines, tris, poses, S):
    """cfs_clearance_mesh_motion of one problem.  lines: (nline, 6) rows (static); tris: (nt, 3, 3) per mesh; poses: (H, 4, 4) or
    (H, 3, 4) per mesh.  Returns clearance_reference.audit's namespace over all columns (lines first) plus v_mesh (nmesh, H)."""
    X, U, xR1 = np.asarray(x_, float).reshape(H, 2 * nj), np.asarray(u, float).reshape(H, nj), np.asarray(xR1, float)
    nline, nobs = len(lines), len(lines) + len(tris)
    TH, _ = CR.samples(H, nj, dt, x_, u, xR1, np.zeros((1, 6)), S)
    itvs = [intervals(t, p, dt) for t, p in zip(tris, poses)]
    D, LK = _distances(O, robot, TH, lines, tris, itvs, S)
    v_mesh = np.array([[it.v for it in iv] for iv in itvs]).reshape(len(tris), H)
    rho = CR.rho_matrix(robot, nj)
    L = np.zeros((H, S, nobs))
    for i in range(H):
        v0 = xR1[nj:] if i == 0 else X[i - 1, nj:]
        vo = np.concatenate([np.zeros(nline), v_mesh[:, i]])
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
                           L_max=L.reshape(-1, nobs).max(axis=0), D=D, v_mesh=v_mesh, i_path=i_min, k_path=k_min)


def dense_min(O, robot, H, nj, dt, x_, u, xR1, lines, tris, poses, S):
    """min of dist_arm over the S-sample grid, (nobs,): the stand-in for continuous time in the soundness test"""
    TH, _ = CR.samples(H, nj, dt, x_, u, xR1, np.zeros((1, 6)), S)
    itvs = [intervals(t, p, dt) for t, p in zip(tris, poses)]
    return _distances(O, robot, TH, lines, tris, itvs, S)[0].reshape(-1, len(lines) + len(tris)).min(axis=0)
