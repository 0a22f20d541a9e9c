"""The CPU restatement of RRT in a cell with mesh obstacles (tests/rrt_mesh_reference.py) that the GPU tests compare against:
(i) with no mesh it is oracle/rrt_oracle.py's find_route exactly; (ii) on the scene of the GPU tests no decision of any compared
tree is a close call, which is what makes a comparison bit for bit meaningful (the device evaluates the same geometry without FMA
contraction and through a hierarchy: a distance may differ in its last bits, a decision only within rounding of its threshold).
No GPU here."""
import numpy as np

import rrt_mesh_reference as M


def test_restatement_without_meshes_is_the_rrt_oracle(O):
    from oracle import rrt_oracle as R
    robot = O.robotproperty2("M200i")
    line, x0, goal, rg, rs, ratial = M.scene_numbers()
    for solver, t in (("RRT", 0), ("RRT*", 1)):
        u = R.splitmix_uniforms(M.SEED, t, M.NDRAW)
        want = R.find_route(robot, [line], x0, goal, goal, rg, rs, np.zeros(5), ratial, R.ArrayRng(u), solver, max_iter=150)
        got = M.find_route(O, robot, [line], [], x0, goal, goal, rg, rs, np.zeros(5), ratial, R.ArrayRng(u), solver, max_iter=150)
        for k in ("route", "all_nodes", "total_dis", "all_ee"):
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{solver} tree {t}: {k}")
        assert (got["node_num"], got["fail_code"], got["proposals"]) == (want["node_num"], want["fail_code"], want["proposals"])
        assert got["closest_call"] == np.inf and got["mesh_rejects"] == 0


def test_no_compared_tree_of_the_scene_has_a_close_call():
    """Trees 0-3 of the scene, both solvers (the trees tests/test_gpu_rrt_mesh.py compares bit for bit): every tree's closest call is
    above 1e-7 m -- rounding moves a distance of this size (metres) by about 1e-15 -- and in every tree the mesh decides: it rejects
    proposals the lines let through.  A changed scene that weakens the comparison fails here."""
    jobs = [(s, t) for s in ("RRT", "RRT*") for t in range(4)]
    res = M.trees(jobs)
    for (s, t), r in zip(jobs, res):
        print(f"[{s} tree {t}] nodes {r['node_num']} fail {r['fail_code']} proposals {r['proposals']} mesh rejects {r['mesh_rejects']} "
              f"closest call {r['closest_call']:.3e} m")
    for (s, t), r in zip(jobs, res):
        assert r["closest_call"] > 1e-7, (s, t, r["closest_call"])
        assert r["mesh_rejects"] >= 1, (s, t)
