"""Cases shared by the tests of the clearance audit with mesh obstacles (tests/test_gpu_clearance_mesh.py on the device,
tests/test_clearance_mesh_reference.py on the CPU): main_FANUC.m's problem with the 488-triangle post and ball of
tests/test_gpu_mesh.py::_mesh_problem next to / instead of its line obstacle, in the product's and in the oracle's form."""
import numpy as np

from motionplanning_5d_m_amd import mesh as M

MESH_ID = 9                                            # oracle mesh slots 0..8 belong to the other test modules


def post_and_ball(with_line):
    """(488, 3, 3) triangles: a post with a ball on top, moved aside when the reference's line obstacle stays"""
    tri = np.concatenate([M.cylinder_mesh((3.606, 8.413), 0.03, 0.0, 0.95, nseg=12, nring=6),
                          M.icosphere([3.606, 8.413, 1.0], 0.06, subdiv=2)])
    return tri + np.array([-0.25, 0.55, -0.3]) if with_line else tri


def oracle_cell(O, obs, tri, with_line, mesh_id=MESH_ID):
    """the oracle's obs cell (the mesh as its NaN-flagged `l`) and the same as (nobs, 6) rows for clearance_reference.audit"""
    l = O.mesh_register(mesh_id, tri)
    cell = ([dict(l=o["l"], D=o["D"], epsilon=o["epsilon"]) for o in obs] if with_line else []) + [dict(l=l, D=0.2, epsilon=0.25)]
    rows = np.stack([np.concatenate([np.asarray(o["l"], float)[:, 0], np.asarray(o["l"], float)[:, 1]]) for o in cell])
    return cell, rows


def pose_of(TH, S, dt, t_path):
    """the pose of the sample at time t_path, from clearance_reference.samples' TH (H, S+1, nj): sample k = 1..S of interval i
    (t = (i + k/S) dt), or the start pose at t = 0"""
    g = int(round(t_path / dt * S))
    return TH[0, 0] if g == 0 else TH[(g - 1) // S, (g - 1) % S + 1]
