"""The cases of tests/test_family_host.py: case files for tests/native/family_check.cpp (flat arrays of doubles in the layout that
program documents), built from exact small fractions and the Python builder of sys_info, and how one case is run.
tests/tools/record_family_host.py records them."""
import os
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np

from motionplanning_5d_m_amd import sysinfo

CFS, PSGCFS = 0, 1
OPS = ["create", "weights", "cost", "poses"]        # first entry of a stored case file
SHAPES = {1: (2, 3, 0.5), 2: (3, 4, 0.1), 3: (6, 2, 0.25)}   # case -> nj, H, dt


def _mat(n, m, a, b, mod):
    """an n x m matrix of small exact fractions: entry (i, j) = ((a i + b j) mod `mod`) / mod - 1/2"""
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    return ((a * i + b * j) % mod) / float(mod) - 0.5


def weights(case):
    nj = SHAPES[case][0]
    Qp = np.diag(1.0 + np.arange(nj))
    Qv = np.diag(2.0 + 0.5 * np.arange(nj))
    Rblk = np.diag(3.0 + np.arange(nj)) + 0.25 * np.eye(nj, k=1)          # not symmetric: R + R' symmetrises it
    if case == 1:
        Rblk = np.diag(3.0 + np.arange(nj))
    return dict(Qp=Qp, Qv=Qv, q_cross=0.1, w_stage=0.1, w_terminal=10000.0, Rblk=Rblk, cR=10.0)


def sys_info(case):
    nj, H, dt = SHAPES[case]
    w = weights(case)
    return sysinfo.build_sys_info(SimpleNamespace(delta_t=dt), nj, H, np.zeros(nj), np.ones(nj), np.zeros(H * 2 * nj), Qp=w["Qp"], Qv=w["Qv"],
                                  Rblk=w["Rblk"], cR=w["cR"], lim=np.ones(nj), max_input_blk=np.ones(nj), epsilon_O=1e-3, MAX_O_ITER=2)


def f_order(M):
    return np.asarray(M, float).ravel(order="F")


def create_case(case, mode, QQ, Aaug=None, Baug=None):
    nj, H, dt = SHAPES[case]
    parts = [np.array([nj, H, mode, dt, Aaug is not None, Baug is not None], float), f_order(QQ)]
    parts += [f_order(M) for M in (Aaug, Baug) if M is not None]
    return "create", np.concatenate(parts)


def weights_case(case, want_alpha):
    nj, H, dt = SHAPES[case]
    w = weights(case)
    head = np.array([nj, H, dt, want_alpha, w["q_cross"], w["w_stage"], w["w_terminal"], w["cR"]], float)
    return "weights", np.concatenate([head, f_order(w["Qp"]), f_order(w["Qv"]), f_order(w["Rblk"])])


def cost_case(case, Qaug):
    nj, H, dt = SHAPES[case]
    return "cost", np.concatenate([np.array([nj, H, dt], float), f_order(Qaug)])


def box(lo, hi):
    """the 12 triangles of an axis-aligned box, 12 x 9"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    v = np.array([[(hi if (k >> a) & 1 else lo)[a] for a in range(3)] for k in range(8)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tri = []
    for a, b, c, d in quads:
        tri += [np.concatenate([v[a], v[b], v[c]]), np.concatenate([v[a], v[c], v[d]])]
    return np.array(tri)


def rot(axis, theta):
    a = np.asarray(axis, float)
    a = a / np.sqrt(a @ a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(theta) * K + (1 - np.cos(theta)) * (K @ K)


def pose(R, t):
    return np.hstack([np.asarray(R, float), np.asarray(t, float).reshape(3, 1)]).ravel()


def poses_case(pose_rows, dt=0.5):
    """one mesh (the box), H = 3"""
    tri = box([0.1, -0.2, 0.0], [0.5, 0.3, 0.4])
    return "poses", np.concatenate([np.array([1, 3, dt], float), np.array([len(tri)], float), tri.ravel(), np.concatenate(pose_rows)])


def cases():
    out = {}
    for case in (1, 2, 3):
        s = sys_info(case)
        modes = {"cfs": CFS, "psgcfs": PSGCFS} if case != 2 else {"cfs": CFS}
        QQ = s.QQ
        if case == 2:                                  # the dense path with a QQ that is not symmetric: the library symmetrises it
            n = QQ.shape[0]
            QQ = QQ + 0.01 * np.triu(_mat(n, n, 3, 5, 17), 1)
        for name, mode in modes.items():
            out[f"create_{case}_{name}"] = create_case(case, mode, QQ, s.Aaug, s.Baug)
        out[f"weights_{case}_alpha"] = weights_case(case, 1)
        if case == 1:
            out["weights_1_noalpha"] = weights_case(case, 0)
        out[f"cost_{case}"] = cost_case(case, s.Qaug_state)
    nx = SHAPES[2][1] * 2 * SHAPES[2][0]
    G = _mat(nx, nx, 5, 7, 23)
    out["cost_2_dense"] = cost_case(2, G @ G.T + 0.05 * _mat(nx, nx, 2, 9, 13))          # a full, non-symmetric Qaug
    # refusals of the dense path
    s = sys_info(1)
    n = s.QQ.shape[0]
    indef = s.QQ.copy(); indef[n - 1, n - 1] = -1.0
    nan = s.QQ.copy(); nan[1, 2] = np.nan
    out["refuse_qq_indefinite"] = create_case(1, CFS, indef)
    out["refuse_qq_zero"] = create_case(1, CFS, np.zeros_like(s.QQ))
    out["refuse_qq_nan"] = create_case(1, CFS, nan)
    Bbad = s.Baug.copy(); Bbad[7, 2] += 1e-9
    Abad = s.Aaug.copy(); Abad[4, 2] += 1e-9
    out["refuse_baug"] = create_case(1, CFS, s.QQ, s.Aaug, Bbad)
    out["refuse_aaug"] = create_case(1, CFS, s.QQ, Abad, s.Baug)
    # poses, H = 3
    I = pose(np.eye(3), np.zeros(3))
    R = rot([1.0, 2.0, 3.0], 0.3)
    T1 = pose(R, [0.2, -0.1, 0.05])
    T2 = pose(rot([1.0, 2.0, 3.0], 0.5), [0.25, -0.1, 0.1])
    out["poses_identity"] = poses_case([I, I, I])
    out["poses_turn"] = poses_case([I, T1, T2])
    out["poses_held"] = poses_case([T1, T1.copy(), T2])
    out["poses_quarter"] = poses_case([I, pose(rot([0.0, 0.0, 1.0], 1.7), [0.0, 0.0, 0.0]), T2])
    out["refuse_pose_reflection"] = poses_case([I, pose(np.diag([1.0, 1.0, -1.0]), np.zeros(3)), I])
    out["refuse_pose_scale"] = poses_case([I, I, pose((1.0 + 1e-6) * R, np.zeros(3))])
    bad = T1.copy(); bad[7] = np.nan
    out["refuse_pose_nan"] = poses_case([bad, I, I])
    return out


def run(program, op, data):
    """(result array, refusal line or None) of one case"""
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        np.asarray(data, float).tofile(fin)
        r = subprocess.run([program, op, fin, fout], capture_output=True, text=True, check=True)
        line = r.stdout.strip()
        return np.fromfile(fout, dtype=np.float64), (line if line.startswith("REFUSED") else None)
