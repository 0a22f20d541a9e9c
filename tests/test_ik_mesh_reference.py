"""The CPU restatement of inverse kinematics with mesh obstacles (tests/ik_mesh_reference.py) and the scene it fixes for the GPU tests.

No device: with no mesh the restatement is ik_reference.solve bit for bit; the scene of tests/test_gpu_ik_mesh.py has the properties
that keep the GPU tests from passing trivially -- every kind of target occurs and no converged restart comes within 1e-7 m of a
threshold, the margin tests/test_rrt_mesh_reference.py guarantees for the same decision."""
import numpy as np

import ik_mesh_reference as K
import ik_reference as R
import rrt_mesh_reference as M


def test_without_a_mesh_it_is_the_line_restatement_bit_for_bit(O):
    arm, lim, lines, tri, inp = K.scene()
    obs, D = K.obs_rows(lines)
    kw = dict(restarts=8, max_iter=inp.max_iter, tol_pos=inp.tol_pos, tol_axis=inp.tol_axis, seed=K.SEED, obs=obs, D=D)
    t = K.KIND_C
    want = R.solve(arm, inp.target_pos[t], inp.target_axis[t][None], inp.theta_ref[t], lim[:, 0], lim[:, 1], **kw)
    got = K.solve(O, arm, inp.target_pos[t], inp.target_axis[t][None], inp.theta_ref[t], lim[:, 0], lim[:, 1], **kw)
    for k in vars(want):
        np.testing.assert_array_equal(getattr(got, k), getattr(want, k), err_msg=k)
    assert np.isposinf(got.cand_closest).all() and not got.cand_mesh_hit.any()


def test_the_scene_of_the_gpu_tests(O):
    arm, lim, lines, tri, inp = K.scene()
    assert tri.shape == (160, 3, 3) and len(lines) == 1 and lines[0]["D"] == 0.2 and M.CYL_D == 0.1
    assert inp.target_pos.shape == (K.T_SCENE, 3) and K.T_SCENE >= 5 and K.RESTARTS == 64
    for q in inp.q:                                                          # poses of configurations near the cylinder
        pos = O.arm_pos(arm.robot, q)
        dm, _, _ = O.mesh_seg_distance(K.MESH_ID, np.concatenate([pos[:, 0], pos[:, 1]], axis=1))
        assert dm.min() < K.NEAR
        assert (q > lim[:, 0]).all() and (q < lim[:, 1]).all()
    mesh = K.scene_solution(True)
    line = K.without_meshes(mesh, inp.theta_ref)
    kinds = K.kinds(line, mesh)
    conv = mesh.cand_mesh_hit | (mesh.cand_status == 0)
    print(f"[ik mesh scene] kinds {kinds}; converged and past the line {int(conv.sum())} of {conv.size}, rejected by the cylinder "
          f"{int(mesh.cand_mesh_hit.sum())}; closest call {mesh.cand_closest.min():.3e} m")
    assert kinds[K.KIND_B] == "b" and kinds[K.KIND_C] == "c" and kinds[K.KIND_A_PLATE] == "c"
    assert mesh.cand_closest.min() >= 1e-7
    # kind (a): the two-mesh cell (cylinder + plate), target KIND_A_PLATE
    two = K.scene_solution(True, plate=True, only=K.KIND_A_PLATE)
    line_a = K.without_meshes(two, inp.theta_ref[K.KIND_A_PLATE][None])
    assert K.kinds(line_a, two) == ["a"]
    assert line_a.selected[0] == line.selected[K.KIND_A_PLATE]                      # the plate leaves the line-only answer alone
    assert two.cand_closest.min() >= 1e-7
    free = np.nonzero(two.cand_status[0] == 0)[0]
    print(f"[ik mesh scene] kind (a): line-only winner {line_a.selected[0]} rejected, restart {two.selected[0]} wins; {free.size} free, "
          f"{int(two.cand_mesh_hit.sum())} rejected; closest call {two.cand_closest.min():.3e} m")
    assert np.isfinite(two.clearance[0]) and two.clearance[0] >= 0


def test_the_reference_map_case_leaves_out_no_restart(O):
    """the deep-hierarchy case of tests/test_gpu_ik_mesh.py on the CPU: for the chosen seed no converged restart of the reference comes
    within 1e-7 m of the threshold (a restart may be left out only below 1e-9 m), and the map decides both ways"""
    arm, lim, D, tri, inp = K.map_case()
    assert tri.shape[0] == 13258 and D == 0.2 and inp.target_pos.shape == (3, 3)
    ref = K.map_solution()
    conv = ref.cand_mesh_hit | (ref.cand_status == 0)
    print(f"[ik mesh map] converged {int(conv.sum())} of {conv.size}, rejected by the map {int(ref.cand_mesh_hit.sum())}, free "
          f"{int((ref.cand_status == 0).sum())}; closest call {ref.cand_closest.min():.3e} m; status {ref.status.tolist()}")
    assert ref.cand_closest.min() >= 1e-7
    assert int((ref.cand_closest < 1e-9).sum()) == 0                          # left out: none
    assert ref.cand_mesh_hit.any() and (ref.cand_status == 0).any()
