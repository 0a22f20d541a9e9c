"""Inverse kinematics against mesh obstacles on the GPU (cfs_ik_solve_mesh*, IKSolver with mesh entries, plan_to_pose(ik_meshes=True)).

The iteration is checked against the line-only call (bit for bit), the decision per restart against the brute-force host rule
(tests/ik_mesh_reference.mesh_rule: oracle.mesh_seg_distance over every triangle, no hierarchy) applied to the device's OWN
cand_theta, the clearance against cfs_dist_arm / cfs_dist_arm_mesh, the selection against the restated cost.  Scene and kinds of
targets: tests/ik_mesh_reference.py (asserted on the CPU by tests/test_ik_mesh_reference.py).

Shapes: T = 1, 3 (one wave of the workgroup has no target), 5 (a second, partly filled workgroup); restarts 64 and 7 (idle lanes)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import ik_mesh_reference as K
import ik_reference as R
import rrt_mesh_reference as M
from test_gpu_ik import _check_selection

pytestmark = pytest.mark.gpu
VARIANTS = ["per_lane", "wave", "small_frontier"]
OUT = ("theta", "status", "selected", "n_ok", "err_pos", "err_axis", "clearance", "cand_theta", "cand_status", "cand_iter")
PLATE_ID = K.PLATE_ID          # oracle mesh slot of the second mesh


def _overflows(reset=False):
    from motionplanning_5d_m_amd import _lib
    n = C.c_ulonglong(0)
    _lib.check(_lib.lib().cfs_debug_ik_frontier_overflows(C.byref(n), 1 if reset else 0))
    return int(n.value)


@pytest.fixture(scope="module")
def scene(gpu, O):
    arm, lim, lines, tri, inp = K.scene()
    return arm, lim, lines, gpu.Mesh(tri=tri), inp


def _solver(gpu, name, obs, restarts, inp=None, variant=None, nj=None):
    kw = dict(max_iter=inp.max_iter, tol_pos=inp.tol_pos, tol_axis=inp.tol_axis) if inp is not None else dict(tol_pos=1e-6, tol_axis=1e-6)
    return gpu.IKSolver(gpu.robotproperty2(name), obs, restarts=restarts, mesh_variant=variant, njoint=nj, **kw)


def _same(a, b, tag, skip=()):
    for k in OUT:
        if k not in skip:
            np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=f"{tag}: {k}")


def _check_decisions(O, name, sol, line, meshes, tag, allow=0.0):
    """rules 1 and 2: the iteration is the line-only call's; cand_status is its cand_status except 0 -> 2 exactly where the brute-force
    rule on the device's own cand_theta says a mesh rejects the pose.  Returns (restarts tested, rejected, left out)."""
    np.testing.assert_array_equal(sol.cand_theta, line.cand_theta, err_msg=f"{tag}: cand_theta")
    np.testing.assert_array_equal(sol.cand_iter, line.cand_iter, err_msg=f"{tag}: cand_iter")
    robot = O.robotproperty2(name)
    tested = rejected = left = 0
    for t, k in np.ndindex(*line.cand_status.shape):
        if line.cand_status[t, k] != 0:
            assert sol.cand_status[t, k] == line.cand_status[t, k], (tag, t, k)
            continue
        hit, closest, _ = K.mesh_rule(O, robot, sol.cand_theta[t, k], meshes)
        tested, rejected = tested + 1, rejected + int(hit)
        if sol.cand_status[t, k] != (2 if hit else 0):
            assert sol.cand_status[t, k] in (0, 2) and closest < 1e-9, (tag, t, k, sol.cand_status[t, k], hit, closest)
            left += 1
    print(f"[ik mesh {tag}] converged and past the lines {tested}, rejected by a mesh {rejected}, left out {left}")
    assert left <= allow * tested
    return tested, rejected, left


def _check_clearance(gpu, name, sol, lines, meshes, tag):
    """rule 5: min(line clearance, cfs_dist_arm_mesh - D_mesh) to 1e-12 m, >= 0; NaN rows for unsolved targets.  meshes: [(Mesh, D)]"""
    ok = np.nonzero(sol.status == 0)[0]
    bad = sol.status != 0
    assert np.isnan(sol.theta[bad]).all() and (sol.selected[bad] == -1).all() and np.isnan(sol.clearance[bad]).all()
    if not ok.size:
        return 0.0
    robot = gpu.robotproperty2(name)
    want = np.full(ok.size, np.inf)
    if lines:
        d, _ = gpu.dist_arm(robot, sol.theta[ok], gpu.obs_to_array(lines))
        want = (d - np.array([o["D"] for o in lines])[None, :]).min(axis=1)
    for m, D in meshes:
        dm, _, _ = gpu.dist_arm_surf(robot, sol.theta[ok], m)
        want = np.minimum(want, dm - D)
    err = float(np.abs(sol.clearance[ok] - want).max())
    print(f"[ik mesh {tag}] clearance of {ok.size} solved targets: max |device - restated| = {err:.2e} m, min clearance {sol.clearance[ok].min():.4f} m")
    assert err <= 1e-12 and (sol.clearance[ok] >= 0).all()
    return err


# ---- 1. 2. 4. 5. every shape, every flag setting ---------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("T,restarts", [(1, 64), (3, 64), (5, 64), (1, 7), (3, 7), (5, 7)])
def test_iteration_decision_selection_and_clearance(gpu, O, scene, T, restarts, variant):
    arm, lim, lines, mesh, inp = scene
    order = [K.KIND_A_PLATE, K.KIND_B, K.KIND_C] + [t for t in range(K.T_SCENE) if t not in (K.KIND_A_PLATE, K.KIND_B, K.KIND_C)]
    idx = order[:T]
    tp, ta, tref = inp.target_pos[idx], inp.target_axis[idx], inp.theta_ref[idx]
    line = _solver(gpu, "M200i", lines, restarts, inp).solve(tp, ta, tref, seed=K.SEED, want_candidates=True)
    sol = _solver(gpu, "M200i", lines + [dict(mesh=mesh, D=M.CYL_D)], restarts, inp, variant).solve(tp, ta, tref, seed=K.SEED, want_candidates=True)
    tag = f"T={T} R={restarts} {variant}"
    _check_decisions(O, "M200i", sol, line, [(K.MESH_ID, M.CYL_D)], tag)           # at most 0 left out on the chosen scene
    _check_selection(sol, tref)
    _check_clearance(gpu, "M200i", sol, lines, [(mesh, M.CYL_D)], tag)


# ---- 3. fails without the feature ------------------------------------------------------------------------------------------------
def test_the_three_kinds_of_targets(gpu, O, scene):
    arm, lim, lines, mesh, inp = scene
    line = _solver(gpu, "M200i", lines, K.RESTARTS, inp).solve(inp.target_pos, inp.target_axis, inp.theta_ref, seed=K.SEED, want_candidates=True)
    sol = _solver(gpu, "M200i", lines + [dict(mesh=mesh, D=M.CYL_D)], K.RESTARTS, inp).solve(inp.target_pos, inp.target_axis, inp.theta_ref,
                                                                                         seed=K.SEED, want_candidates=True)
    a, b, c = K.KIND_A_PLATE, K.KIND_B, K.KIND_C
    # (a) lives in the two-mesh cell (cylinder + plate): tests/ik_mesh_reference.py says why
    plate = gpu.Mesh(tri=K.plate_triangles())
    two = _solver(gpu, "M200i", lines + [dict(mesh=mesh, D=M.CYL_D), dict(mesh=plate, D=K.PLATE["D"])], K.RESTARTS, inp).solve(
        inp.target_pos, inp.target_axis, inp.theta_ref, seed=K.SEED, want_candidates=True)
    assert line.status[a] == 0 and two.status[a] == 0 and two.selected[a] != line.selected[a]
    assert two.cand_status[a, line.selected[a]] == 2
    for m, D in ((mesh, M.CYL_D), (plate, K.PLATE["D"])):
        dm, _, _ = gpu.dist_arm_surf(gpu.robotproperty2("M200i"), two.theta[a][None], m)
        assert dm[0] >= D
    assert line.status[b] == 0 and sol.status[b] == 2 and sol.selected[b] == -1 and sol.n_ok[b] == 0
    assert np.isnan(sol.theta[b]).all() and np.isnan(sol.err_pos[b]) and np.isnan(sol.err_axis[b]) and np.isnan(sol.clearance[b])
    assert line.status[c] == 0
    for k in OUT:
        if k != "clearance":
            np.testing.assert_array_equal(getattr(sol, k)[c], getattr(line, k)[c], err_msg=k)


# ---- 6. the variants ---------------------------------------------------------------------------------------------------------------
def test_variants_agree_bit_for_bit_and_the_overflow_path_runs(gpu, scene):
    arm, lim, lines, mesh, inp = scene
    obs = lines + [dict(mesh=mesh, D=M.CYL_D)]
    res, over = {}, {}
    for v in [None] + VARIANTS:
        _overflows(reset=True)
        res[v] = _solver(gpu, "M200i", obs, K.RESTARTS, inp, v).solve(inp.target_pos, inp.target_axis, inp.theta_ref, seed=K.SEED, want_candidates=True)
        over[v] = _overflows()
    for v in VARIANTS:
        _same(res[v], res[None], f"{v} vs default")
    print(f"[ik mesh variants] frontier overflows: {over}")
    assert over["per_lane"] == 0 and over["wave"] == 0 and over[None] == 0 and over["small_frontier"] > 0


# ---- 7. obstacle columns -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["per_lane", "wave"])
def test_two_meshes_and_no_line_obstacle(gpu, O, scene, variant):
    arm, lim, lines, mesh, inp = scene
    tri = K.plate_triangles()
    O.mesh_register(PLATE_ID, tri)
    plate = gpu.Mesh(tri=tri)
    idx = [K.KIND_A_PLATE, K.KIND_B, K.KIND_C]
    tp, ta, tref = inp.target_pos[idx], inp.target_axis[idx], inp.theta_ref[idx]
    for obs_lines, tag in ((lines, "two meshes"), ([], "no line")):
        cell = [dict(mesh=mesh, D=M.CYL_D)] + ([dict(mesh=plate, D=K.PLATE["D"])] if obs_lines else [])
        ids = [(K.MESH_ID, M.CYL_D)] + ([(PLATE_ID, K.PLATE["D"])] if obs_lines else [])
        line = _solver(gpu, "M200i", obs_lines or None, 64, inp).solve(tp, ta, tref, seed=K.SEED, want_candidates=True)
        sol = _solver(gpu, "M200i", obs_lines + cell, 64, inp, variant).solve(tp, ta, tref, seed=K.SEED, want_candidates=True)
        _check_decisions(O, "M200i", sol, line, ids, f"{tag} {variant}")
        _check_selection(sol, tref)
        _check_clearance(gpu, "M200i", sol, obs_lines, [(c["mesh"], c["D"]) for c in cell], f"{tag} {variant}")
        if not obs_lines:
            assert np.isposinf(line.clearance[line.status == 0]).all() and np.isfinite(sol.clearance[sol.status == 0]).all()


# ---- 8. other joint counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nj,axis", [("M16iB", 6, True), ("2L", 2, False)])
def test_other_joint_counts(gpu, O, name, nj, axis):
    """a plate through the middle of the last link of a configuration q, theta_ref = q: restart 0 converges at q without an iteration
    and the plate rejects it (chosen on the CPU: the brute-force rule says so before the device is asked)"""
    lim = gpu.robotproperty2(name).thetamax[:nj]
    robot = O.robotproperty2(name)
    arm = R.Arm(robot, nj)
    q = R.in_limit_configs(lim, 2, 91)
    pos = O.arm_pos(robot, q[0])
    tri = K.plate_triangles(0.5 * (pos[nj - 1, 0] + pos[nj - 1, 1]), half=0.05)
    O.mesh_register(PLATE_ID, tri)
    assert K.mesh_rule(O, robot, q[0], [(PLATE_ID, 0.03)])[0]
    poses = [arm.pose(x) for x in q]
    tp, ta = np.array([p for p, _ in poses]), np.array([a for _, a in poses])
    plate = gpu.Mesh(tri=tri)
    line = _solver(gpu, name, None, 64, nj=nj).solve(tp, ta if axis else None, q, seed=4, want_candidates=True)
    for variant in ("per_lane", "wave"):
        sol = _solver(gpu, name, [dict(mesh=plate, D=0.03)], 64, variant=variant, nj=nj).solve(tp, ta if axis else None, q, seed=4, want_candidates=True)
        tested, rejected, _ = _check_decisions(O, name, sol, line, [(PLATE_ID, 0.03)], f"{name} {variant}")
        assert rejected >= 1 and sol.cand_status[0, 0] == 2 and line.cand_status[0, 0] == 0
        _check_selection(sol, q)
        _check_clearance(gpu, name, sol, [], [(plate, 0.03)], f"{name} {variant}")


# ---- 9. a deep hierarchy -----------------------------------------------------------------------------------------------------------
def test_reference_map(gpu, O):
    """tests/test_ik_mesh_reference.py asserts without a device that the reference leaves out no restart of this case for K.SEED"""
    arm, lim, D, tri, inp = K.map_case()
    w = SimpleNamespace(D=D)
    mesh = gpu.Mesh(tri=tri)
    tp, ta, tref = inp.target_pos, inp.target_axis, inp.theta_ref
    line = _solver(gpu, "M200i", None, 64, inp).solve(tp, ta, tref, seed=K.SEED, want_candidates=True)
    res = {}
    for variant in VARIANTS:
        _overflows(reset=True)
        res[variant] = _solver(gpu, "M200i", [dict(mesh=mesh, D=w.D)], 64, inp, variant).solve(tp, ta, tref, seed=K.SEED, want_candidates=True)
        print(f"[ik mesh map {variant}] frontier overflows {_overflows()}")
        _check_decisions(O, "M200i", res[variant], line, [(K.MAP_ID, w.D)], f"map {variant}", allow=0.02)
        _check_clearance(gpu, "M200i", res[variant], [], [(mesh, w.D)], f"map {variant}")
    assert (res["wave"].cand_status != line.cand_status).any()                 # the map rejected something
    _same(res["per_lane"], res["wave"], "map A vs B")
    _same(res["small_frontier"], res["wave"], "map small frontier vs B")


# ---- 10. batch independence and determinism ------------------------------------------------------------------------------------------
def test_batch_independence_and_determinism(gpu, scene):
    import torch
    arm, lim, lines, mesh, inp = scene
    slv = _solver(gpu, "M200i", lines + [dict(mesh=mesh, D=M.CYL_D)], K.RESTARTS, inp)
    a = K.KIND_A_PLATE
    rep = lambda x, n: np.repeat(x[a][None], n, axis=0)  # noqa: E731
    alone = slv.solve(inp.target_pos[a], inp.target_axis[a], inp.theta_ref[a], seed=K.SEED, want_candidates=True)
    for T, pos in ((3, 2), (130, 77)):
        tp, ta, tr = rep(inp.target_pos, T), rep(inp.target_axis, T), rep(inp.theta_ref, T)
        for x, src in ((tp, inp.target_pos), (ta, inp.target_axis), (tr, inp.theta_ref)):
            x[:pos] = src[K.KIND_B]
            x[pos + 1:] = src[K.KIND_C]
        big = slv.solve(tp, ta, tr, seed=K.SEED, want_candidates=True)
        for k in OUT:
            np.testing.assert_array_equal(getattr(big, k)[pos], getattr(alone, k)[0], err_msg=f"T={T}: {k}")
    again = slv.solve(tp, ta, tr, seed=K.SEED, want_candidates=True)
    _same(again, big, "twice")
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    td = lambda x: torch.tensor(x, dtype=torch.float64, device=dev)  # noqa: E731
    got = slv.solve_device(td(tp), td(ta), td(tr), seed=K.SEED, want_candidates=True, stream=side)
    side.synchronize()
    for k in OUT:
        np.testing.assert_array_equal(getattr(got, k).cpu().numpy(), getattr(big, k), err_msg=f"side stream: {k}")


# ---- 11. the planner ---------------------------------------------------------------------------------------------------------------
def test_plan_to_pose_with_mesh_obstacles(gpu, O, scene):
    import torch
    arm, lim, lines, mesh, inp = scene
    pobs, s, g, region_g, region_s, off = gpu.RRTstar_problem()
    S = 4
    planner = gpu.RRTCFSPlanner([pobs[0], dict(mesh=mesh, D=M.CYL_D, epsilon=M.CYL_D)], s, region_g, region_s, off, num_seed=2, max_slots=S)
    idx = [K.KIND_A_PLATE, K.KIND_C, K.KIND_B, K.KIND_C]
    tp, ta = inp.target_pos[idx], inp.target_axis[idx]
    x0 = np.broadcast_to(np.asarray(s.x0, float), (S, 5)).copy()
    with pytest.raises(ValueError, match="ik_meshes"):
        planner.plan_to_pose(x0, tp, ta, seed=3)
    res = planner.plan_to_pose(x0, tp, ta, seed=3, ik_meshes=True)
    st = res.ik_status.cpu().numpy()
    assert st[2] == 2 and int(res.status[2]) == -2 and (st[[0, 1, 3]] == 0).all()
    goal = res.goal.cpu().numpy()
    robot = O.robotproperty2("M200i")
    for t in (0, 1, 3):
        assert not K.mesh_rule(O, robot, goal[t], [(K.MESH_ID, M.CYL_D)])[0]
    found = np.where(st[:, None] == 0, goal, x0)
    ref = planner.plan(x0, found, 3)
    for k, v in vars(ref).items():
        if isinstance(v, torch.Tensor) and k not in ("status", "has_solution", "selected"):
            assert np.array_equal(getattr(res, k).cpu().numpy(), v.cpu().numpy(), equal_nan=True), k
    for k in ("status", "has_solution", "selected"):
        assert torch.equal(getattr(res, k)[[0, 1, 3]], getattr(ref, k)[[0, 1, 3]]), k
    planner.close()
