"""Lifetime of the problem handle's device state (csrc/cfs_host.h DevBuf, csrc/cfs_problem.h): a handle that has had its mesh set,
its mesh motion, the audits' workspace and pose table and every optional buffer allocated, grown, replaced and dropped answers, bit
for bit, what a fresh handle answers.  Nothing here measures free device memory (it is device-wide); that every buffer is freed
once is what the types say.

Shape: main_FANUC (M200i, nj = 5) at H = 4, one line obstacle and one mesh (nobs = 2), max_batch = 2; m1 is a 12-triangle box
where the post of the mesh-motion tests stands, m2 the far box."""
import numpy as np
import pytest

import mesh_motion_reference as M
from test_gpu_mesh_motion import _Cell

pytestmark = pytest.mark.gpu
H, B = 4, 2
SOLVE = ("u", "x_", "cost_all", "e_cost_all", "e_u_all", "iter_O", "total_iter", "status")
AUDIT = ("dist_wp", "dist_path", "dist_lower", "t_path", "link_path", "tri_path", "short_by")


def _m1(gpu):
    cx, cy = M.C_POST
    return gpu.mesh.box_mesh([cx - 0.03, cy - 0.03, -0.3], [cx + 0.03, cy + 0.03, 0.65], n=1)


def _answers(c, poses):
    """a solve and a clearance_mesh of the static handle, then a solve and a clearance_mesh_motion with `poses`"""
    out = []
    r = c.solve()
    out += [getattr(r, k) for k in SOLVE]
    a = c.h.clearance_mesh(r.x_, r.u, c.xR1, c.obs, substeps=3)
    out += [getattr(a, k) for k in AUDIT]
    c.h.set_mesh_motion([poses])
    r = c.solve()
    out += [getattr(r, k) for k in SOLVE]
    a = c.h.clearance_mesh_motion(r.x_, r.u, c.xR1, c.obs, substeps=3)
    out += [getattr(a, k) for k in AUDIT]
    return out


def _toggles(c, soften):
    """every optional buffer of the handle allocated, replaced and dropped, twice; soften only while the handle has no meshes"""
    h = c.h
    for _ in range(2):
        h.set_state_cost(c.s.Qaug_state)
        if soften:
            h.set_infeasible_policy("soften", 1e4)
            h.set_infeasible_policy("stop")
        h.stamps(B)
        h.stamps(0)
        h.trace(0, cap=16)
        h.trace(0, cap=0)
        h.log_u(True)
        h.log_u(False)
        h.log_u(True)


@pytest.mark.parametrize("rep,mode", [(0, "CFS"), (1, "PSGCFS"), (2, "CFS")])
def test_a_worn_handle_answers_like_a_fresh_one(gpu, rep, mode):
    s = M.fanuc(gpu, H)
    poses, other = M.poses_z(H, 0.05, 0.3), M.poses_general(H, 0.03, 0.2)
    c = _Cell(gpu, s, mode, [_m1(gpu)], B=B)                  # 1. set_meshes([m1]) ...
    m1, m2 = c.meshes[0], gpu.Mesh(tri=M.far_box(gpu.mesh))
    h = c.h
    r = c.solve()                                             #    ... then solve
    _toggles(c, False)
    audit = lambda entry, S: getattr(h, entry)(r.x_, r.u, c.xR1, c.obs, substeps=S)   # noqa: E731
    small = audit("clearance_mesh", 2)                        # 2. the second call grows the workspace
    audit("clearance_mesh", 5)
    for k in AUDIT:
        np.testing.assert_array_equal(getattr(audit("clearance_mesh", 2), k), getattr(small, k), err_msg=k)
    _toggles(c, False)
    h.set_mesh_motion([poses])                                # 3.
    small = audit("clearance_mesh_motion", 2)                 # 4. the second call grows the pose table
    audit("clearance_mesh_motion", 4)
    _toggles(c, False)
    h.set_mesh_motion([other])                                # 5. the table is rebuilt: the answer is the other poses', and differs
    moved = audit("clearance_mesh_motion", 2)
    assert not np.array_equal(moved.dist_path[:, 1], small.dist_path[:, 1])
    h.set_mesh_motion([poses])
    for k in AUDIT:
        np.testing.assert_array_equal(getattr(audit("clearance_mesh_motion", 2), k), getattr(small, k), err_msg=k)
    h.set_mesh_motion(None)                                   # 6.
    h.set_meshes([])                                          #    no meshes: the only state in which soften is admitted
    _toggles(c, True)
    h.set_meshes([m2])                                        # 7.
    c.solve()
    _toggles(c, False)
    h.set_meshes([m1])                                        # 8.
    got = _answers(c, poses)

    fresh = _Cell(gpu, s, mode, [_m1(gpu)], B=B)
    want = _answers(fresh, poses)
    assert len(got) == len(want) == 2 * (len(SOLVE) + len(AUDIT))
    for k, (x, y) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(x, y, err_msg=f"answer {k}")
    fresh.close()
    c.close()
    c.close()                                                 # twice is harmless
    h.close()
    m2.close()
