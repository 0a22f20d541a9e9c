"""The certified bound of the clearance audit holds against a faceted surface with v_obs = 0 (include/cfs_hip.h,
cfs_clearance_mesh), checked on the CPU: the test-side reference (tests/clearance_reference.py), whose
oracle distance measures a mesh when an obstacle row starts with NaN, audits the oracle's CFS and PSGCFS solutions of the two
main_FANUC mesh cases; dist_lower(16) of the mesh column lies below a 256-step dense sampling and is as tight as its definition."""
import numpy as np
import pytest

import clearance_mesh_cases as MC
import clearance_reference as CR


@pytest.fixture(scope="module")
def solved(O, golden):
    out = {}
    for with_line in (True, False):
        P = O.problem_main_FANUC()
        tri = MC.post_and_ball(with_line)
        cell, rows = MC.oracle_cell(O, P.obs, tri, with_line)
        for mode in ("CFS", "PSGCFS"):
            nz = golden["main_FANUC_PSGCFS/noise"] if mode == "PSGCFS" else None
            w = O.optimizer(P.ROBOT, P.sys_info, cell, mode, noise=nz)
            out[with_line, mode] = (P, tri, rows, w)
    return out


@pytest.mark.parametrize("mode", ["CFS", "PSGCFS"])
@pytest.mark.parametrize("with_line", [True, False])
def test_bound_holds_on_a_faceted_surface(O, solved, with_line, mode):
    P, tri, rows, w = solved[with_line, mode]
    O.mesh_register(MC.MESH_ID, tri)                   # the slot is shared by the two cases
    s = P.sys_info
    robot, dt = O.robotproperty2("M200i"), s.robot.delta_t
    xR1 = np.asarray(s.xR1, float).reshape(-1)
    args = (O, robot, s.H, 5, dt, w.x_, w.u, xR1, rows)
    a = {S: CR.audit(*args, S) for S in (8, 16, 32)}
    dense = CR.dense_min(*args, 256)
    jm = rows.shape[0] - 1                             # the mesh column
    assert np.isnan(rows[jm, 0])
    print(f"with_line={with_line} {mode}: mesh column dist_wp {a[16].dist_wp[jm]:.7f} dist_path {a[16].dist_path[jm]:.7f} "
          f"dist_lower {a[16].dist_lower[jm]:.7f} dense(256) {dense[jm]:.7f}")
    assert (a[16].dist_lower <= dense).all(), a[16].dist_lower - dense
    assert (dense <= a[16].dist_path).all() and (a[16].dist_path <= a[16].dist_wp).all()
    for S in (8, 16, 32):
        gap = a[S].dist_path - a[S].dist_lower
        assert (gap >= 0).all() and (gap <= a[S].L_max * dt / (2 * S)).all(), (S, gap, a[S].L_max * dt / (2 * S))
    assert np.abs(a[16].D).min() > 2e-4                # no sample is near the surrogate
