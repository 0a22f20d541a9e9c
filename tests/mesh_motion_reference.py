"""Test-side reference of moving mesh obstacles (include/cfs_hip.h, cfs_problem_set_mesh_motion), built on the
oracle's own primitives in the way tests/moving_reference.py is.  Collision row (j, i) of get_con depends only on waypoint i's pose
and on obstacle j, so for waypoint i every moving mesh is registered with the oracle where pose [j][i] puts it (its triangles
transformed on the host in double: no inverse pose, no hierarchy), one oracle get_con is taken, and waypoint i's rows are kept.  The
oracle's mesh registry is global, so this runs sequentially.  The outer loop is tests/reference_loop.py's with this get_con.
Used by tests/test_mesh_motion_reference.py (which validates it and vets the cases) and tests/test_gpu_mesh_motion.py."""
from types import SimpleNamespace

import numpy as np

import reference_loop as RL

D_MARGIN, EPS_MARGIN = 0.2, 0.25                 # main_FANUC's margins: obs.D (PSGCFS) and obs.epsilon (CFS)
C_POST = (3.356, 8.963)                          # the vertical the post stands on
FIRST_ID = 8                                     # oracle mesh ids FIRST_ID + j hold mesh j of the cell being measured


# ---- poses -----------------------------------------------------------------------------------------------------------------------
def rot(axis, ang):
    """Rodrigues: rotation by ang about the unit vector along `axis`"""
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(ang) * K + (1.0 - np.cos(ang)) * (K @ K)


def pose_about(axis, pivot, ang, trans):
    """4x4: rotate by ang about the line through `pivot` along `axis`, then translate by `trans`"""
    T = np.eye(4)
    R, p = rot(axis, ang), np.asarray(pivot, float)
    T[:3, :3], T[:3, 3] = R, p - R @ p + np.asarray(trans, float)
    return T


def poses_z(H, dy, ang, c=C_POST):
    """(H, 4, 4): at waypoint i+1, f = (i+1)/H: a rotation by ang*f about the vertical through c, then a translation (0, dy*f, 0)"""
    return np.stack([pose_about([0, 0, 1], [c[0], c[1], 0.0], ang * (i + 1) / H, [0.0, dy * (i + 1) / H, 0.0]) for i in range(H)])


def poses_general(H, dy, ang, c=C_POST):
    """(H, 4, 4): the same schedule about the axis (1, 2, 3)/sqrt(14) through a pivot 0.3 m off the post: all nine entries of R"""
    pivot = [c[0] + 0.3, c[1], 0.3]
    return np.stack([pose_about([1, 2, 3], pivot, ang * (i + 1) / H, [0.0, dy * (i + 1) / H, 0.0]) for i in range(H)])


def identity_poses(H):
    return np.broadcast_to(np.eye(4), (H, 4, 4)).copy()


def transform(tri, T):
    """(nt, 3, 3) triangles placed by the 4x4 (or 3x4) pose T, in double"""
    T = np.asarray(T, float)
    return np.asarray(tri, float) @ T[:3, :3].T + T[:3, 3]


# ---- geometry --------------------------------------------------------------------------------------------------------------------
def uv_sphere(center, radius, nseg=10, nring=6):
    """nseg x nring UV sphere; the degenerate halves of the pole quads are left out (the surface is the same point set)"""
    th = np.linspace(0.0, np.pi, nring + 1)
    ph = np.arange(nseg + 1) * (2 * np.pi / nseg)
    P = np.stack([np.outer(np.sin(th), np.cos(ph)), np.outer(np.sin(th), np.sin(ph)), np.outer(np.cos(th), np.ones_like(ph))], -1)
    P[0], P[-1] = [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]
    P[:, -1] = P[:, 0]
    tri = []
    for k in range(nring):
        for i in range(nseg):
            a, b, c, d = P[k, i], P[k + 1, i], P[k + 1, i + 1], P[k, i + 1]
            if k < nring - 1:
                tri.append([a, b, c])
            if k > 0:
                tri.append([a, c, d])
    return np.asarray(center, float) + radius * np.asarray(tri)


def post_and_ball(mesh_mod, off, c=C_POST):
    """the post (a 12-gon prism, radius 0.03, z -0.3 .. 0.65, capped) with a ball (radius 0.06) at (c_x + off, c_y, 0.7)"""
    return np.concatenate([mesh_mod.cylinder_mesh(c, 0.03, -0.3, 0.65, nseg=12, nring=1), uv_sphere([c[0] + off, c[1], 0.7], 0.06)])


def far_box(mesh_mod):
    """a box the arm never comes near: the mesh that is held still"""
    return mesh_mod.box_mesh([2.2, 9.9, 0.0], [2.4, 10.1, 0.3], n=1)


# ---- the problem: main_FANUC at horizon H ------------------------------------------------------------------------------------------
X0 = np.array([0.7825, 0.0284, 0.2172, 0.1444, -1.1779])
XG = np.array([-0.7825, 0.0284, 0.2172, 0.1444, -1.1779])
LINE = np.array([[3806, 8413, 1], [3606, 8413, 1038]], float).T / 1000        # main_FANUC's line obstacle


def fanuc(mod, H):
    """main_FANUC.m's sys_info at horizon H from `mod` (the oracle module or the package: same build_sys_info)"""
    robot = mod.robotproperty2("M200i")
    Qp = np.diag([10.0, 10.0, 1.0, 1.0, 1.0])
    Rblk = np.array([[10.0, 0, 0, 0, 0], [0, 10, 1, 0, 0], [0, 1, 2, 0, 0], [0, 0, 0, 2, 0], [0, 0, 0, 0, 1]])
    s = mod.build_sys_info(robot, 5, H, X0, XG, mod.line_reference(X0, XG, H), Qp=Qp, Qv=Qp, Rblk=Rblk, cR=50.0, lim=np.ones(5),
                           max_input_blk=np.array([1, 1, np.pi, np.pi, np.pi]) * robot.delta_t, epsilon_O=1e-1, MAX_O_ITER=20)
    s.xR1 = np.concatenate([X0, np.zeros(5)])
    return s


def noise_rows(H):
    return np.random.default_rng(2).standard_normal((20, H * 5)) * 0.1


# ---- get_con and the outer loop ----------------------------------------------------------------------------------------------------
def _cell(O, lines, tris, poses, i):
    """the oracle's obs cell at waypoint i: the line obstacles, then every mesh registered where its pose puts it"""
    cell = [dict(l=l, D=D_MARGIN, epsilon=EPS_MARGIN) for l in lines]
    for j, (tri, T) in enumerate(zip(tris, poses)):
        cell.append(dict(l=O.mesh_register(FIRST_ID + j, transform(tri, T[i])), D=D_MARGIN, epsilon=EPS_MARGIN))
    return cell


def get_con_posed(O, ROBOT, s, lines, tris, poses, x_, u, mode):
    """get_con with mesh j placed by poses[j][i] at waypoint i.  lines: 3x2 axes; tris: (nt, 3, 3) per mesh; poses: (H, 4, 4) per
    mesh; s needs xR1.  Returns (Ainq, binq, dist (nobs, H), linkid (nobs, H), grad (nobs, H, nj)) in the reference's row order."""
    H, nj = s.H, s.njoint
    nobs, per = len(lines) + len(tris), 1 + 2 * nj
    A, b = np.zeros((nobs * H * per, H * nj)), np.zeros(nobs * H * per)
    dist, lid, grad = np.zeros((nobs, H)), np.zeros((nobs, H), np.int32), np.zeros((nobs, H, nj))
    for i in range(H):
        Ai, bi, di, li, gi = O.get_con(ROBOT, s, _cell(O, lines, tris, poses, i), x_, u, mode=mode)
        for j in range(nobs):
            r = slice((j * H + i) * per, (j * H + i + 1) * per)
            A[r], b[r] = Ai[r], bi[r]
        dist[:, i], lid[:, i], grad[:, i] = di[:, i], li[:, i], gi[:, i]
    return A, b, dist, lid, grad


def optimizer_posed(O, ROBOT, s, lines, tris, poses, mode, x_init, noise=None):
    """CFS_FANUC / PSGCFS_FANUC .optimizer() of one problem against meshes placed per waypoint: reference_loop.optimizer with
    get_con_posed"""
    return RL.optimizer(O, ROBOT, s, mode, lambda s2, x_, u: get_con_posed(O, ROBOT, s2, lines, tris, poses, x_, u, mode),
                        x_init, s.xR1, s.ff, s.caug, noise=noise)


def clearance_where_it_is(O, s, tris, poses, x_):
    """min over the waypoints of the oracle's dist_arm between waypoint i's arm and every mesh where pose i puts it"""
    th = np.asarray(x_, float).reshape(s.H, 2 * s.njoint)[:, :s.njoint]
    d = np.inf
    for i in range(s.H):
        for j, (tri, T) in enumerate(zip(tris, poses)):
            d = min(d, O.dist_arm(s.robot, th[i], O.mesh_register(FIRST_ID + j, transform(tri, T[i])))[0])
    return d


CASES = SimpleNamespace(                                  # (H, off, dy, ang) of the vetted cases
    lin=(30, 0.05, -0.3, 0.6), cfs12=(12, 0.0, -0.1, 0.6), cfs30=(30, 0.0, -0.1, 0.6), psg=(30, 0.05, -0.3, 0.6))
