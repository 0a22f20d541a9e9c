"""Batched collision-aware inverse kinematics on the GPU (cfs_ik_solve, cfs_tool_pose, RRTCFSPlanner.plan_to_pose) against the
oracle's forward kinematics, cfs_dist_arm, the selection rule restated in numpy and the CPU restatement tests/ik_reference.py.

Shapes: T = 1, 3, 130 (more targets than the 4 of one workgroup, and not a multiple of it); restarts 1, 7 (a partly filled wave)
and 64; M200i (5 joints) and M16iB (6) with and without the axis, 2L (2) position only.  Targets are oracle poses of seeded random
configurations inside the joint ranges: reachable by construction.  Position-only answers lie on a 2-D set and where a restart stops
on it is ill-conditioned, so theta parity with the restatement is asserted in axis mode only; position-only mode is covered by the
independent properties and the selection rule."""
import numpy as np
import pytest

import ik_reference as R

pytestmark = pytest.mark.gpu

TOL = 1e-6
ROBOTS = [("M200i", 5, True), ("M200i", 5, False), ("M16iB", 6, True), ("M16iB", 6, False), ("2L", 2, False)]


def _targets(O, pkg, name, nj, T, seed):
    lim = pkg.robotproperty2(name).thetamax[:nj]
    arm = R.Arm(O.robotproperty2(name), nj)
    q = R.in_limit_configs(lim, 4 * T + 8, seed)
    if name == "M200i":                                                      # configurations that clear _obstacle by 5 cm themselves
        d, _ = pkg.dist_arm(pkg.robotproperty2(name), q, pkg.obs_to_array(_obstacle(pkg)))
        q = q[d[:, 0] - _obstacle(pkg)[0]["D"] >= 0.05]
    q = q[:T]
    assert q.shape[0] == T
    poses = [arm.pose(x) for x in q]
    return arm, lim, q, np.array([p for p, _ in poses]), np.array([a for _, a in poses])


def _obstacle(pkg):
    # a line obstacle well inside the M200i's workspace: some restarts end in collision, others do not
    return [dict(l=np.array([[3.4, 3.4], [8.3, 8.3], [0.0, 1.2]]), D=0.08)]


def _check_solved(O, pkg, name, arm, lim, sol, tp, ta, obs):
    """item 2 for every solved target"""
    robot = pkg.robotproperty2(name)
    ok = np.nonzero(sol.status == 0)[0]
    for t in ok:
        th = sol.theta[t]
        p, a = arm.pose(th)
        ep = np.linalg.norm(p - tp[t])
        ea = np.linalg.norm(a - ta[t]) if ta is not None else 0.0
        assert ep <= TOL + 1e-12 and ea <= TOL + 1e-12, (name, t, ep, ea)
        assert abs(sol.err_pos[t] - ep) <= 1e-12 and abs(sol.err_axis[t] - ea) <= 1e-12, (sol.err_pos[t], ep, sol.err_axis[t], ea)
        assert (th >= lim[:, 0]).all() and (th <= lim[:, 1]).all()
    if obs and ok.size:
        d, _ = pkg.dist_arm(robot, sol.theta[ok], pkg.obs_to_array(obs))
        want = (d - np.array([o["D"] for o in obs])[None, :]).min(axis=1)
        assert np.abs(sol.clearance[ok] - want).max() <= 1e-12
        assert (sol.clearance[ok] >= 0).all()
    else:
        assert np.isposinf(sol.clearance[ok]).all()
    bad = sol.status != 0
    assert np.isnan(sol.theta[bad]).all() and (sol.selected[bad] == -1).all() and np.isnan(sol.err_pos[bad]).all() and np.isnan(sol.clearance[bad]).all()


def _check_selection(sol, tref, w=None):
    """item 3: theta is cand_theta[selected] bit for bit, selected the first argmin of the weighted distance over state 0"""
    T, Rr, nj = sol.cand_theta.shape
    w = np.ones(nj) if w is None else w
    for t in range(T):
        ok = np.nonzero(sol.cand_status[t] == 0)[0]
        assert sol.n_ok[t] == ok.size
        if ok.size == 0:
            assert sol.selected[t] == -1 and np.isnan(sol.theta[t]).all() and sol.status[t] in (1, 2)
            assert sol.status[t] == (2 if (sol.cand_status[t] == 2).any() else 1)
            continue
        assert sol.status[t] == 0
        cost = []
        for k in ok:
            c_ = 0.0
            for c in range(nj):
                dlt = float(sol.cand_theta[t, k, c]) - float(tref[t, c])
                c_ = c_ + float(w[c]) * (dlt * dlt)
            cost.append(c_)
        cost = np.array(cost)
        k = sol.selected[t]
        assert k in ok
        np.testing.assert_array_equal(sol.theta[t], sol.cand_theta[t, k])
        assert k == ok[int(np.argmin(cost))], (t, k, cost)                   # the first minimum; the cost is plain IEEE in joint order


@pytest.mark.parametrize("name,nj", [("M200i", 5), ("M16iB", 6), ("2L", 2)])
def test_tool_pose_parity(gpu, O, name, nj):
    arm, lim, q, tp, ta = _targets(O, gpu, name, nj, 7, seed=21)
    robot = gpu.robotproperty2(name)
    pos, dr, jac = gpu.tool_pose(robot, q, want_jac=True)
    assert np.abs(pos - tp).max() <= 1e-12 and np.abs(dr - ta).max() <= 1e-12
    h = 1e-6
    for n in range(q.shape[0]):
        for c in range(nj):
            e = np.zeros(nj)
            e[c] = h
            pp, ap = arm.pose(q[n] + e)
            pm, am = arm.pose(q[n] - e)
            assert np.abs(jac[n, :, c] - np.concatenate([pp - pm, ap - am]) / (2 * h)).max() <= 1e-7
    _, _, ends = gpu.dist_arm(robot, q, np.zeros((1, 6)), want_pos=True)
    np.testing.assert_array_equal(pos, ends[:, nj - 1, 0])                # the default tool is the last capsule's first end
    # another tool: a point off the axis and a tilted direction
    tool, axis = np.array([0.03, -0.02, 0.05]), np.array([0.3, -0.5, 0.8])
    arm2 = R.Arm(O.robotproperty2(name), nj, tool, axis)
    pos2, dr2 = gpu.tool_pose(robot, q, tool=tool, tool_axis=axis)
    want = [arm2.pose(x) for x in q]
    assert np.abs(pos2 - np.array([p for p, _ in want])).max() <= 1e-12 and np.abs(dr2 - np.array([a for _, a in want])).max() <= 1e-12


@pytest.mark.parametrize("name,nj,axis", ROBOTS)
@pytest.mark.parametrize("T,restarts", [(1, 64), (3, 7), (130, 64)])
def test_solved_targets_and_selection(gpu, O, name, nj, axis, T, restarts):
    arm, lim, q, tp, ta = _targets(O, gpu, name, nj, T, seed=31 + T)
    obs = _obstacle(gpu) if name == "M200i" else None
    slv = gpu.IKSolver(gpu.robotproperty2(name), obs, restarts=restarts, tol_pos=TOL, tol_axis=TOL)
    tref = np.broadcast_to(0.5 * (lim[:, 0] + lim[:, 1]), (T, nj))
    sol = slv.solve(tp, ta if axis else None, tref, seed=5, want_candidates=True)
    print(f"[ik {name} axis={axis} T={T} R={restarts}] solved {int((sol.status == 0).sum())}/{T}, restarts converged "
          f"{(sol.cand_status == 0).mean():.2f}, in collision {(sol.cand_status == 2).mean():.2f}, numeric {int((sol.cand_status == 3).sum())}")
    _check_solved(O, gpu, name, arm, lim, sol, tp, ta if axis else None, obs)
    _check_selection(sol, tref)
    assert (sol.cand_theta >= lim[None, None, :, 0]).all() and (sol.cand_theta <= lim[None, None, :, 1]).all()
    assert (sol.cand_status != 3).all()
    if restarts == 64:
        assert (sol.status == 0).mean() >= 0.9                              # reachable, collision-free targets and 64 starts


def test_one_restart_at_theta_ref_converges_without_an_iteration(gpu, O):
    arm, lim, q, tp, ta = _targets(O, gpu, "M200i", 5, 3, seed=41)
    tref = q.copy()
    tref[1, 0] = lim[0, 1] + 0.3                                             # outside: restart 0 starts at the clamped value
    q[1, 0] = lim[0, 1]
    tp[1], ta[1] = arm.pose(q[1])
    for restarts in (1, 7):
        slv = gpu.IKSolver(gpu.robotproperty2("M200i"), restarts=restarts, tol_pos=TOL, tol_axis=TOL)
        sol = slv.solve(tp, ta, tref, seed=3, want_candidates=True)
        assert (sol.status == 0).all() and (sol.selected == 0).all() and (sol.cand_iter[:, 0] == 0).all() and (sol.cand_status[:, 0] == 0).all()
        np.testing.assert_array_equal(sol.cand_theta[:, 0], q)                # the clamped theta_ref, untouched
        np.testing.assert_array_equal(sol.theta, q)
        assert sol.cand_theta.shape == (3, restarts, 5)


def test_one_target_one_restart_position_only_without_the_optional_outputs(gpu, O):
    """cfs_ik_solve's staging at its edges: nobs = 0 (zero-length obs / D), T = 1, restarts = 1, use_axis = 0 (target_axis NULL), every
    optional output NULL.  The restart starts at theta_ref, the pose of its own target: theta_ref comes back bit for bit, as above."""
    import ctypes as C
    from motionplanning_5d_m_amd import _lib
    arm, lim, q, tp, ta = _targets(O, gpu, "M200i", 5, 1, seed=41)
    slv = gpu.IKSolver(gpu.robotproperty2("M200i"), restarts=1, tol_pos=TOL, tol_axis=TOL)
    d = slv._desc(False, 3, slv.obs, slv.D)
    assert d.nobs == 0 and d.use_axis == 0 and d.restarts == 1
    theta, status = np.full((1, 5), 7.0), np.full(1, 7, np.int32)
    o = _lib.cfs_ik_out()
    o.theta, o.status = theta.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)
    assert not (o.selected or o.n_ok or o.err_pos or o.err_axis or o.clearance or o.cand_theta or o.cand_status or o.cand_iter)
    tp1, tr1 = np.ascontiguousarray(tp[:1]), np.ascontiguousarray(q[:1])
    _lib.check(_lib.lib().cfs_ik_solve(C.byref(d), 1, tp1.ctypes.data_as(C.c_void_p), None, tr1.ctypes.data_as(C.c_void_p), C.byref(o)))
    assert status[0] == 0
    np.testing.assert_array_equal(theta, q[:1])


def test_tool_pose_of_one_configuration(gpu, O):
    """cfs_tool_pose with N = 1, with jac NULL and with jac given: test_tool_pose_parity's reference and tolerances"""
    arm, lim, q, tp, ta = _targets(O, gpu, "M200i", 5, 1, seed=21)
    robot = gpu.robotproperty2("M200i")
    pos, dr = gpu.tool_pose(robot, q)
    assert pos.shape == (1, 3) and np.abs(pos - tp).max() <= 1e-12 and np.abs(dr - ta).max() <= 1e-12
    pos_j, dr_j, jac = gpu.tool_pose(robot, q, want_jac=True)
    np.testing.assert_array_equal(pos_j, pos)
    np.testing.assert_array_equal(dr_j, dr)
    h = 1e-6
    for c in range(5):
        e = np.zeros(5)
        e[c] = h
        pp, ap = arm.pose(q[0] + e)
        pm, am = arm.pose(q[0] - e)
        assert np.abs(jac[0, :, c] - np.concatenate([pp - pm, ap - am]) / (2 * h)).max() <= 1e-7


def test_parity_with_the_cpu_restatement_in_axis_mode(gpu):
    P = R.PARITY
    lim = gpu.robotproperty2(P["robot"]).thetamax[:P["nj"]]
    arm, inp, ref, out, movement, tol = R.parity_case(lim)
    assert out.mean() <= 0.05
    slv = gpu.IKSolver(gpu.robotproperty2(P["robot"]), restarts=P["restarts"], max_iter=P["max_iter"], tol_pos=P["tol_pos"], tol_axis=P["tol_axis"])
    sol = slv.solve(inp.target_pos, inp.target_axis, inp.theta_ref, seed=P["seed"], want_candidates=True)
    keep = ~out
    np.testing.assert_array_equal(sol.cand_status[keep], ref.cand_status[keep])
    conv = keep & (ref.cand_status == 0)
    diff = np.abs(sol.cand_theta - ref.cand_theta).max(axis=2)
    print(f"[ik parity] {int(conv.sum())} converged restarts compared, left out {int(out.sum())} of {out.size}; max |theta - reference| "
          f"{diff[conv].max():.2e} rad (tolerance {tol:.2e}); iterations equal on {(sol.cand_iter[conv] == ref.cand_iter[conv]).mean():.2f}")
    assert diff[conv].max() <= tol
    np.testing.assert_array_equal(sol.selected, ref.selected)
    np.testing.assert_array_equal(sol.status, ref.status)


def test_infeasible_targets(gpu, O):
    robot = gpu.robotproperty2("M200i")
    arm, lim, q, tp, ta = _targets(O, gpu, "M200i", 5, 2, seed=51)
    reach = sum(np.hypot(robot.DH[j, 2], robot.DH[j, 1]) for j in range(5)) + 1.0
    far = robot.base + np.array([reach, 0.0, 0.0])
    slv = gpu.IKSolver(robot, restarts=64, tol_pos=TOL, tol_axis=TOL)
    sol = slv.solve(np.vstack([tp, far]), None, None, seed=1, want_candidates=True)
    assert sol.status[2] == 1 and sol.n_ok[2] == 0 and (sol.cand_status[2] == 1).all() and sol.selected[2] == -1 and np.isnan(sol.theta[2]).all()
    assert (sol.status[:2] == 0).all()
    # an obstacle axis through a reachable target point: every restart that reaches the point is in collision
    pt = tp[0]
    obs = [dict(l=np.stack([pt - np.array([0, 0, 0.5]), pt + np.array([0, 0, 0.5])], axis=1), D=0.3)]
    hit = gpu.IKSolver(robot, obs, restarts=64, tol_pos=TOL, tol_axis=TOL).solve(tp[:1], None, None, seed=1, want_candidates=True)
    assert hit.status[0] == 2 and np.isin(hit.cand_status[0], (1, 2)).all() and (hit.cand_status[0] == 2).any() and hit.selected[0] == -1
    free = slv.solve(tp[:1], None, None, seed=1)
    assert free.status[0] == 0


def test_results_do_not_depend_on_the_batch_and_are_deterministic(gpu, O):
    import torch
    arm, lim, q, tp, ta = _targets(O, gpu, "M200i", 5, 130, seed=61)
    slv = gpu.IKSolver(gpu.robotproperty2("M200i"), _obstacle(gpu), restarts=64, tol_pos=TOL, tol_axis=TOL)
    tref = R.in_limit_configs(lim, 130, seed=62)
    big = slv.solve(tp, ta, tref, seed=9, want_candidates=True)
    again = slv.solve(tp, ta, tref, seed=9, want_candidates=True)
    names = ("theta", "status", "selected", "n_ok", "err_pos", "err_axis", "clearance", "cand_theta", "cand_status", "cand_iter")
    for k in names:
        np.testing.assert_array_equal(getattr(big, k), getattr(again, k), err_msg=k)
    for rows in ([129], [5, 129, 64], [0]):                                  # alone, in a batch of 3 (other positions), first
        part = slv.solve(tp[rows], ta[rows], tref[rows], seed=9, want_candidates=True)
        for k in names:
            np.testing.assert_array_equal(getattr(part, k), getattr(big, k)[rows], err_msg=k)
    # device tensors on a side stream behind other work, no host synchronisation in between
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    d = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    tpd, tad, trd = d(tp), d(ta), d(tref)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        busy = torch.ones(2048, 2048, dtype=torch.float64, device=dev)
        for _ in range(4):
            busy = busy @ busy * 1e-4
        got = slv.solve_device(tpd, tad, trd, seed=9, want_candidates=True, stream=side)
    side.synchronize()
    for k in names:
        np.testing.assert_array_equal(getattr(got, k).cpu().numpy(), getattr(big, k), err_msg=k)


def test_plan_to_pose(gpu, O):
    import torch
    pobs, s, g, region_g, region_s, off = gpu.RRTstar_problem()
    S = 8
    planner = gpu.RRTCFSPlanner(pobs, s, region_g, region_s, off, num_seed=2, max_slots=S)
    lim = s.robot.thetamax[:5]
    arm = R.Arm(O.robotproperty2("M200i"), 5)
    rng = np.random.default_rng(71)
    goals = []
    obs6, D = gpu.obs_to_array(pobs), np.array([o["D"] for o in pobs])
    while len(goals) < S:                                                    # goals that RRT's feasible() accepts
        gq = np.asarray(s.goal_th) + 0.15 * (2 * rng.random(5) - 1)
        d, _ = gpu.dist_arm(s.robot, gq[None], obs6)
        if ((d[0] - D) >= 0.02).all() and (gq > lim[:, 0]).all() and (gq < lim[:, 1]).all():
            goals.append(gq)
    poses = [arm.pose(x) for x in goals]
    tp, ta = np.array([p for p, _ in poses]), np.array([a for _, a in poses])
    x0 = np.broadcast_to(np.asarray(s.x0, float), (S, 5)).copy()
    res = planner.plan_to_pose(x0, tp, ta, seed=3)
    assert (res.ik_status.cpu().numpy() == 0).all()
    goal = res.goal.cpu().numpy()
    from types import SimpleNamespace
    sol = SimpleNamespace(err_pos=res.ik_err_pos.cpu().numpy(), clearance=res.ik_clearance.cpu().numpy())
    for t in range(S):
        p, a = arm.pose(goal[t])
        assert np.linalg.norm(p - tp[t]) <= 1e-6 + 1e-12 and np.linalg.norm(a - ta[t]) <= 1e-6 + 1e-12
        assert abs(sol.err_pos[t] - np.linalg.norm(p - tp[t])) <= 1e-12
        assert (goal[t] >= lim[:, 0]).all() and (goal[t] <= lim[:, 1]).all()
    d, _ = gpu.dist_arm(s.robot, goal, obs6)
    assert np.abs(sol.clearance - (d - D[None]).min(axis=1)).max() <= 1e-12 and (sol.clearance >= 0).all()
    ref = planner.plan(x0, goal, 3)
    keys = [k for k, v in vars(ref).items() if isinstance(v, torch.Tensor)]
    assert {"u", "x_", "status", "has_solution", "selected", "route", "cost"} <= set(keys)
    for k in keys:
        assert torch.equal(getattr(res, k), getattr(ref, k)) or (torch.isnan(getattr(ref, k)).any() and
                                                                   np.array_equal(getattr(res, k).cpu().numpy(), getattr(ref, k).cpu().numpy(), equal_nan=True)), k
    # one slot whose target is out of reach: masked, the others unchanged
    tp2 = tp.copy()
    tp2[3] = s.robot.base + np.array([5.0, 0.0, 0.0])
    res2 = planner.plan_to_pose(x0, tp2, ta, seed=3)
    assert int(res2.ik_status[3]) == 1 and int(res2.status[3]) == -2 and int(res2.has_solution[3]) == 0 and int(res2.selected[3]) == -1
    assert torch.isnan(res2.goal[3]).all()
    others = [i for i in range(S) if i != 3]
    for k in ("u", "x_", "status", "has_solution", "selected", "goal", "ik_status"):
        assert np.array_equal(getattr(res2, k)[others].cpu().numpy(), getattr(res, k)[others].cpu().numpy(), equal_nan=True), k
    planner.close()
