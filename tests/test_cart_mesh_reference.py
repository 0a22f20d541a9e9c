"""The CPU restatement of Cartesian paths against mesh obstacles (tests/cart_mesh_reference.py) and what its scenes hold, without a
device: with no row rejected it is cart_reference.trace bit for bit; rule 3 on every rejected candidate; the kinds (a)-(f) the GPU
tests rely on; and the threshold margin that lets the GPU tests leave out no candidate -- over every row the restatement tests in every
scene of tests/test_gpu_cart_mesh.py, no (mesh, link) distance comes within 1e-6 m of its threshold, while the device's rows differ
from the restatement's by at most 8.9e-9 rad."""
import numpy as np
import pytest

import cart_mesh_reference as CM
import cart_reference as CR
import ik_mesh_reference as K
from oracle import oracle as O

FIELDS = ("theta", "status", "path", "selected", "n_ok", "n_done", "cand_status", "cand_done", "cand_iter", "cand_end", "cand_path")


def test_with_no_row_rejected_it_is_the_line_only_answer_bit_for_bit():
    arm, lim, lines, tri, inp = CM.scene()
    line = CM.scene_line(2, 64)
    st, _ = CM.scene_starts(64)
    O.mesh_register(K.PLATE_ID, K.plate_triangles(center=(50.0, 50.0, 50.0)))          # a plate nothing reaches
    got = CM.apply_meshes(O, arm.robot, line, st, inp.theta_ref, [(K.PLATE_ID, 0.05)])
    assert (got.cand_m == -1).all()
    for k in FIELDS:
        np.testing.assert_array_equal(getattr(got, k), getattr(line, k), err_msg=k)
    np.testing.assert_array_equal(got.clearance, line.clearance)                       # the far plate never is the minimum
    assert (line.status == 0).any()


@pytest.mark.parametrize("steps", CM.SHAPES_K)
def test_rule_3_on_every_rejected_candidate(steps):
    line, got = CM.scene_line(steps, 64), CM.scene_solution(steps, 64)
    np.testing.assert_array_equal(got.cand_iter, line.cand_iter)                       # rule 4
    hit = 0
    for t, r in np.ndindex(*got.cand_m.shape):
        m = got.cand_m[t, r]
        if m < 0:                                                                      # rule 2
            for k in ("cand_status", "cand_done", "cand_end", "cand_path"):
                np.testing.assert_array_equal(getattr(got, k)[t, r], getattr(line, k)[t, r])
            continue
        hit += 1
        assert not np.isnan(line.cand_path[t, r, m]).any()                              # an accepted row
        assert got.cand_status[t, r] == 2 and got.cand_done[t, r] == max(m - 1, 0)
        np.testing.assert_array_equal(got.cand_end[t, r], line.cand_path[t, r, m])
        assert np.isnan(got.cand_path[t, r, m:]).all()
        np.testing.assert_array_equal(got.cand_path[t, r, :m], line.cand_path[t, r, :m])
    assert hit > 0
    for t in range(CM.T_SCENE):                                                        # rule 5 on the new states
        ok = np.nonzero(got.cand_status[t] == 0)[0]
        assert got.n_ok[t] == ok.size and got.n_done[t] == got.cand_done[t].max()
        if ok.size:
            st, _ = CM.scene_starts(64)
            cost = [float(np.sum((st[t, r] - CM.scene()[4].theta_ref[t]) ** 2)) for r in ok]
            assert got.status[t] == 0 and abs(cost[list(ok).index(got.selected[t])] - min(cost)) <= 1e-12
            np.testing.assert_array_equal(got.path[t], got.cand_path[t, got.selected[t]])
        else:
            assert got.status[t] == 1 and got.selected[t] == -1 and np.isnan(got.path[t]).all() and np.isnan(got.clearance[t])


def test_the_scenes_hold_every_kind():
    line = CM.scene_line(16, 64)
    cyl, two = CM.scene_solution(16, 64), CM.scene_solution(16, 64, plate=True)
    have, have2 = CM.kinds(line, cyl), CM.kinds(line, two)
    print(f"[cart mesh reference] kinds: cylinder {sorted(have)}, cylinder + plate {sorted(have2)}")
    assert {"a", "b", "d", "e", "f"} <= have and "c" in have2
    # the targets the scene names: 0 and 3 enter the margin mid-line, 1 starts inside it, 2 is untouched, 4 only the plate touches
    assert (cyl.cand_m[0] >= 1).any() and (cyl.cand_m[3] >= 1).any() and set(cyl.cand_m[1]) == {-1, 0}
    assert (cyl.cand_m[2] == -1).all() and (cyl.cand_m[4] == -1).all() and (two.cand_m[4] >= 0).any()
    assert line.status[4] == 0 and two.status[4] == 0 and two.selected[4] != line.selected[4] and two.cand_m[4, line.selected[4]] >= 0
    # the clearance of a winner counts the meshes
    ok = cyl.status == 0
    assert ok.any() and (cyl.clearance[ok] <= line.clearance[ok]).all() and (cyl.clearance[ok] >= 0).all()


def test_threshold_margin_of_every_gpu_scene():
    closest = {}
    for steps in CM.SHAPES_K:                                                          # R = 64 holds the candidates of R = 7 and 1, T = 5 every target
        closest[f"cylinder K={steps}"] = CM.scene_solution(steps, 64).cand_closest.min()
    closest["cylinder + plate"] = CM.scene_solution(16, 64, plate=True).cand_closest.min()
    # two meshes and no line obstacle: R = 7, K = 2
    arm, lim, lines, tri, inp = CM.scene()
    st, ss = CM.scene_starts(64)
    line = CR.trace(arm, st[:, :7], inp.target_pos, inp.target_axis, inp.theta_ref, lim[:, 0], lim[:, 1], 2, start_state=ss[:, :7], **CM.CART)
    closest["no line"] = CM.apply_meshes(O, arm.robot, line, st[:, :7], inp.theta_ref, CM.mesh_ids(plate=True)).cand_closest.min()
    for name, nj, axis, _ in CM.JOINTS:
        arm, lim, jin, tri, line = CM.joints_case(name)
        O.mesh_register(K.PLATE_ID, tri)
        got = CM.apply_meshes(O, arm.robot, line, jin.start, jin.theta_ref, [(K.PLATE_ID, CM.JOINTS_D)])
        assert line.cand_status[0, 0] == 0 and got.cand_m[0, 0] >= 0 and got.cand_status[0, 0] == 2
        closest[name] = got.cand_closest.min()
    line, got, _ = CM.map_solution()
    has_rows = ~np.isnan(line.cand_path[:, :, 0, 0])
    assert (got.cand_m >= 0).any() and (got.cand_m[has_rows] < 0).any()                # the map decides both ways
    closest["map"] = got.cand_closest.min()
    print("[cart mesh reference] closest calls (m): " + ", ".join(f"{k} {v:.2e}" for k, v in closest.items()))
    assert min(closest.values()) >= CM.MARGIN
