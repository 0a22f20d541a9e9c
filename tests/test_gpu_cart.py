"""Batched straight-line tool paths on the GPU (cfs_cart_path, CartesianPath, RRTCFSPlanner.plan_to_pose(approach=...)) against
cfs_tool_pose, cfs_dist_arm, the selection rule restated in numpy and the CPU restatement tests/cart_reference.py.

Shapes: T = 1, 3, 130 (130 leaves a workgroup with two idle waves); R = 1, 7 (a partly filled wave) and 64; K = 1, 2, 16; M200i (5
joints) and M16iB (6) with and without the axis, 2L (2) position only; two line obstacles on the M200i, none elsewhere.  Targets are
poses of configurations near the first candidate of their row, so the lines are short and reachable; the other candidates are
configurations near that one and, every fifth, a random one far away (lines that end in joint jumps or steps that do not converge).
The independent properties are checked for every candidate through cand_path; theta parity with the restatement is asserted in
axis mode on the M200i only (isolated solutions: DESIGN.md sections 20 and 23)."""
import numpy as np
import pytest

import cart_reference as CR
import ik_reference as R

pytestmark = pytest.mark.gpu

TOL = 1e-6
ROBOTS = [("M200i", 5, True), ("M200i", 5, False), ("M16iB", 6, True), ("M16iB", 6, False), ("2L", 2, False)]
NAMES = ("theta", "status", "path", "selected", "n_ok", "n_done", "clearance", "cand_status", "cand_done", "cand_iter", "cand_end", "cand_path")


def _obstacles():
    # two line obstacles inside the M200i's workspace: some configurations of a batch touch their margins, most do not
    return [dict(l=np.array([[3.4, 3.4], [8.3, 8.3], [0.0, 1.2]]), D=0.08), dict(l=np.array([[2.2, 3.0], [7.6, 7.6], [0.9, 0.9]]), D=0.05)]


def _case(pkg, name, nj, T, Rn, axis, seed, reach=0.15):
    """starts (T, R, nj), target_pos, target_axis | None, theta_ref"""
    lim = pkg.robotproperty2(name).thetamax[:nj]
    rng = np.random.default_rng(seed)
    q = R.in_limit_configs(lim, T, seed, shrink=0.6)
    start = q[:, None, :] + 0.03 * rng.standard_normal((T, Rn, nj))
    start[:, 0] = q
    far = R.in_limit_configs(lim, T * Rn, seed + 1, shrink=0.9).reshape(T, Rn, nj)
    start[:, 4::5] = far[:, 4::5]
    start = np.clip(start, lim[:, 0], lim[:, 1])
    goal = np.clip(q + reach * (2 * rng.random((T, nj)) - 1), lim[:, 0], lim[:, 1])
    tp, ta = pkg.tool_pose(pkg.robotproperty2(name), goal, njoint=nj)
    tref = R.in_limit_configs(lim, T, seed + 2, shrink=0.6)
    return lim, start, tp, (ta if axis else None), tref


def _line_points(p0, a0, tp, ta, K):
    """(T, R, K+1, 3) line points and axes (None in position-only mode) restated from the header"""
    s = (np.arange(K + 1) / K)[None, None, :, None]
    pk = p0[:, :, None, :] + s * (tp[:, None, None, :] - p0[:, :, None, :])
    if ta is None:
        return pk, None
    tn = ta / np.linalg.norm(ta, axis=1, keepdims=True)
    b = (1.0 - s) * a0[:, :, None, :] + s * tn[:, None, None, :]
    return pk, b / np.linalg.norm(b, axis=3, keepdims=True)


def _check(pkg, name, nj, cp, res, start, tp, ta, tref, obs, start_state=None):
    """the independent properties of every candidate, the reasons of the failed ones, the winner's rows and the selection"""
    with np.errstate(invalid="ignore", divide="ignore"):                    # rows without a start have no line
        _check_body(pkg, name, nj, cp, res, start, tp, ta, tref, obs, start_state)


def _check_body(pkg, name, nj, cp, res, start, tp, ta, tref, obs, start_state):
    robot = pkg.robotproperty2(name)
    T, Rn, K1, _ = res.cand_path.shape
    K, st, done, path = K1 - 1, res.cand_status, res.cand_done, res.cand_path
    lo, hi = cp.lo, cp.hi
    obs6 = pkg.obs_to_array(obs) if obs else None
    Dm = np.array([o["D"] for o in obs]) if obs else None

    def clearance(th):
        if obs6 is None or th.shape[0] == 0:
            return np.full(th.shape[0], np.inf)
        d, _ = pkg.dist_arm(robot, th, obs6)
        return (d - Dm[None, :]).min(axis=1)

    def poses(th):
        return pkg.tool_pose(robot, th, njoint=nj) if th.shape[0] else (np.zeros((0, 3)), np.zeros((0, 3)))
    assert st.min() >= 0 and st.max() <= 5
    # which rows hold configurations: theta_0..theta_done of a candidate whose start was accepted, NaN elsewhere
    have = ~np.isnan(path).any(axis=3)
    assert (have == ~np.isnan(path).all(axis=3)).all()
    row0 = have[:, :, 0]
    assert (have == (row0[:, :, None] & (np.arange(K1)[None, None, :] <= done[:, :, None]))).all()
    assert ((st == 0) == (row0 & (done == K))).all() and (done[~row0] == 0).all()
    np.testing.assert_array_equal(path[:, :, 0][row0], start[row0])
    # no start: exactly the starts the contract refuses
    inside = np.isfinite(start).all(axis=2) & (np.nan_to_num(start) >= lo).all(axis=2) & (np.nan_to_num(start) <= hi).all(axis=2)
    usable = inside if start_state is None else inside & (start_state == 0)
    assert ((st == 5) == ~usable).all()
    assert np.isnan(res.cand_end[st == 5]).all() and (res.cand_iter[st == 5] == 0).all()
    # a start that collides: state 2, nothing done, no row
    hit0 = usable & ~row0
    assert (st[hit0] == 2).all() and (clearance(start[hit0]) < 1e-12).all()
    np.testing.assert_array_equal(res.cand_end[hit0], start[hit0])
    # every accepted configuration: on its line point, inside the limits, free; every step jump-bounded
    p0 = np.zeros((T, Rn, 3))
    a0 = np.zeros((T, Rn, 3))
    p0[row0], a0[row0] = poses(start[row0])
    pk, ak = _line_points(p0, a0, tp, ta, K)
    flat = path[have]
    pos, dr = poses(flat)
    assert np.linalg.norm(pos - pk[have], axis=1).max() <= cp.tol_pos + 1e-12
    if ta is not None:
        assert np.linalg.norm(dr - ak[have], axis=1).max() <= cp.tol_axis + 1e-12
    assert (flat >= lo).all() and (flat <= hi).all()
    cl = np.full((T, Rn, K1), np.inf)
    cl[have] = clearance(flat)
    assert cl.min() >= -1e-12
    step = np.abs(np.diff(path, axis=2)).max(axis=3)
    assert (step[have[:, :, 1:]] <= cp.max_joint_step).all()
    # the stated reason holds at cand_end
    end = res.cand_end
    last = np.take_along_axis(path, done[:, :, None, None].repeat(nj, 3), axis=2)[:, :, 0]     # theta_done
    np.testing.assert_array_equal(end[st == 0], path[:, :, K][st == 0])
    m = (st == 2) & row0
    assert (clearance(end[m]) < 1e-12).all()
    m = st == 4
    assert (np.abs(end[m] - last[m]).max(axis=1) > cp.max_joint_step).all()
    for m in ((st == 2) & row0, st == 4):                                   # these ended ON the next line point
        nxt = np.minimum(done + 1, K)
        pe, de = poses(end[m])
        want_p = np.take_along_axis(pk, nxt[:, :, None, None].repeat(3, 3), axis=2)[:, :, 0][m]
        assert m.sum() == 0 or np.linalg.norm(pe - want_p, axis=1).max() <= cp.tol_pos + 1e-12
    m = st == 1
    if m.any():
        nxt = np.minimum(done + 1, K)
        pe, de = poses(end[m])
        ep = np.linalg.norm(pe - np.take_along_axis(pk, nxt[:, :, None, None].repeat(3, 3), axis=2)[:, :, 0][m], axis=1)
        ea = np.zeros_like(ep) if ta is None else np.linalg.norm(de - np.take_along_axis(ak, nxt[:, :, None, None].repeat(3, 3), axis=2)[:, :, 0][m], axis=1)
        assert ((ep > cp.tol_pos - 1e-12) | (ea > cp.tol_axis - 1e-12)).all()
        assert (res.cand_iter[m] >= cp.max_iter).all()
    # per target: the selection restated to the last bit (first argmin of the cost of the START), and the winner's rows
    w = np.ones(nj) if cp.weight is None else cp.weight
    for t in range(T):
        ok = np.nonzero(st[t] == 0)[0]
        assert res.n_ok[t] == ok.size and res.n_done[t] == done[t].max()
        if ok.size == 0:
            assert res.selected[t] == -1 and res.status[t] == (1 if (st[t] != 5).any() else 2)
            assert np.isnan(res.theta[t]).all() and np.isnan(res.path[t]).all() and np.isnan(res.clearance[t])
            continue
        cost = []
        for r in ok:
            c_ = 0.0
            for c in range(nj):
                dlt = float(start[t, r, c]) - float(tref[t, c])
                c_ = c_ + float(w[c]) * (dlt * dlt)
            cost.append(c_)
        r = res.selected[t]
        assert res.status[t] == 0 and r == ok[int(np.argmin(np.array(cost)))], (t, r, cost)
        np.testing.assert_array_equal(res.theta[t], start[t, r])
        np.testing.assert_array_equal(res.path[t], path[t, r])
        if obs6 is None:
            assert np.isposinf(res.clearance[t])
        else:
            assert abs(res.clearance[t] - cl[t, r].min()) <= 1e-12 and res.clearance[t] >= 0


@pytest.mark.parametrize("name,nj,axis", ROBOTS)
@pytest.mark.parametrize("T,Rn,K", [(1, 64, 16), (3, 7, 2), (130, 64, 16), (130, 1, 1)])
def test_every_candidate_keeps_the_contract(gpu, name, nj, axis, T, Rn, K):
    lim, start, tp, ta, tref = _case(gpu, name, nj, T, Rn, axis, seed=100 + T + Rn)
    obs = _obstacles() if name == "M200i" else None
    cp = gpu.CartesianPath(gpu.robotproperty2(name), obs, steps=K, max_joint_step=0.2 if K > 2 else 0.4)
    res = cp.trace(start, tp, ta, tref, want_candidates=True)
    st = res.cand_status
    print(f"[cart {name} axis={axis} T={T} R={Rn} K={K}] solved {int((res.status == 0).sum())}/{T}, candidate states 0..5 "
          f"{[int((st == s).sum()) for s in range(6)]}, largest cand_iter {int(res.cand_iter.max())}")
    _check(gpu, name, nj, cp, res, start, tp, ta, tref, obs)
    assert (st != 3).all()
    if nj >= 5 or K == 1:                                                    # the short line from the configuration next to the target;
        assert (st[:, 0] == 0).mean() >= 0.5                                 # the 2L's tool moves on a surface that holds no straight chord


def test_zero_length_line(gpu):
    """a target that is the start's own pose: complete without an iteration, every row the start bit for bit"""
    lim, start, tp, ta, tref = _case(gpu, "M200i", 5, 3, 7, True, seed=7)
    robot = gpu.robotproperty2("M200i")
    start[:, :] = start[:, :1]                                               # every candidate of a row is the same configuration
    tp, ta = gpu.tool_pose(robot, start[:, 0])
    for K in (1, 16):
        res = gpu.CartesianPath(robot, steps=K).trace(start, tp, ta, tref, want_candidates=True)
        assert (res.cand_status == 0).all() and (res.cand_iter == 0).all() and (res.cand_done == K).all() and (res.selected == 0).all()
        np.testing.assert_array_equal(res.cand_path, np.broadcast_to(start[:, :, None, :], res.cand_path.shape))
        np.testing.assert_array_equal(res.path, np.broadcast_to(start[:, 0, None, :], res.path.shape))
        np.testing.assert_array_equal(res.cand_end, start)


def test_collision_on_the_line(gpu, O):
    """a line obstacle laid across the tool's line: state 2 at the step the restatement names"""
    robot = gpu.robotproperty2("M200i")
    lim = robot.thetamax[:5]
    arm = R.Arm(O.robotproperty2("M200i"), 5)
    q = R.in_limit_configs(lim, 4, 17, shrink=0.5)
    found = 0
    for x in q:
        p, a = arm.pose(x)
        v = np.cross(a, [0.0, 0.0, 1.0] if abs(a[2]) < 0.9 else [1.0, 0.0, 0.0])
        v /= np.linalg.norm(v)
        mid = p + 0.4 * a                                                    # across the line's extension, 40 cm ahead of the tool point:
        # the last capsule reaches 27 cm beyond its axis, so the start clears the margin by 9 cm and the 20 cm move does not
        obs = [dict(l=np.stack([mid - 0.5 * v, mid + 0.5 * v], axis=1), D=0.04)]
        kw = dict(steps=16, max_iter=20, max_joint_step=0.3, tol_pos=TOL, tol_axis=TOL)
        ref = CR.trace(arm, x[None, None], p + 0.2 * a, a, x, lim[:, 0], lim[:, 1], obs=gpu.obs_to_array(obs), D=np.array([0.04]), **kw)
        if ref.cand_status[0, 0] != 2 or ref.cand_done[0, 0] == 0:
            continue                                                         # this configuration does not make the case
        # the deciding clearances are far from zero, so rounding cannot move the step
        before, after = arm.clearance(ref.cand_path[0, 0, ref.cand_done[0, 0]], gpu.obs_to_array(obs), [0.04]), arm.clearance(
            ref.cand_end[0, 0], gpu.obs_to_array(obs), [0.04])
        if not (before > 1e-6 and after < -1e-6):
            continue
        found += 1
        cp = gpu.CartesianPath(robot, obs, steps=16, max_joint_step=0.3)
        res = cp.trace(x[None, None], p + 0.2 * a, a, x, want_candidates=True)
        assert res.cand_status[0, 0] == 2 and res.status[0] == 1 and res.selected[0] == -1 and res.n_ok[0] == 0
        assert res.cand_done[0, 0] == ref.cand_done[0, 0] and res.n_done[0] == ref.cand_done[0, 0]
        _check(gpu, "M200i", 5, cp, res, x[None, None], (p + 0.2 * a)[None], a[None], x[None], obs)
        free = gpu.CartesianPath(robot, steps=16, max_joint_step=0.3).trace(x[None, None], p + 0.2 * a, a, x, want_candidates=True)
        assert free.cand_status[0, 0] == 0 and np.isposinf(free.clearance[0])
    assert found >= 1


def test_out_of_reach_and_joint_jump(gpu):
    lim, start, tp, ta, tref = _case(gpu, "M200i", 5, 3, 7, True, seed=23)
    robot = gpu.robotproperty2("M200i")
    reach = sum(np.hypot(robot.DH[j, 2], robot.DH[j, 1]) for j in range(5)) + 1.0
    far = np.broadcast_to(robot.base + np.array([reach, 0.0, 0.0]), (3, 3)).copy()
    cp = gpu.CartesianPath(robot, steps=2, max_joint_step=100.0)             # no jump can end a candidate first
    res = cp.trace(start, far, ta, tref, want_candidates=True)
    assert (res.cand_status == 1).all() and (res.status == 1).all() and (res.n_ok == 0).all() and (res.selected == -1).all()
    assert np.isnan(res.theta).all() and np.isnan(res.path).all()
    _check(gpu, "M200i", 5, cp, res, start, far, ta, tref, None)
    start[:, 4] = start[:, 3]                                                # no far candidate: every first step converges
    cj = gpu.CartesianPath(robot, steps=16, max_joint_step=1e-4)
    jump = cj.trace(start, tp, ta, tref, want_candidates=True)
    assert (jump.cand_status == 4).all() and (jump.cand_done == 0).all() and (jump.status == 1).all() and (jump.n_done == 0).all()
    _check(gpu, "M200i", 5, cj, jump, start, tp, ta, tref, None)


def test_no_start(gpu):
    lim, start, tp, ta, tref = _case(gpu, "M200i", 5, 3, 7, True, seed=29)
    robot = gpu.robotproperty2("M200i")
    ss = np.zeros((3, 7), np.int32)
    ss[0, 1], ss[0, 2], ss[0, 3] = 1, 2, 3                                   # IK's states of restarts that did not end free
    start[0, 5, 2] = lim[2, 1] + 1e-9                                        # outside by a hair
    start[0, 6, 0] = np.nan
    start[1, 0, 4] = np.inf
    ss[2, :] = 1                                                             # a target without any start
    cp = gpu.CartesianPath(robot, _obstacles(), steps=2, max_joint_step=0.4)
    res = cp.trace(start, tp, ta, tref, start_state=ss, want_candidates=True)
    assert (res.cand_status[0, [1, 2, 3, 5, 6]] == 5).all() and res.cand_status[1, 0] == 5 and (res.cand_status[2] == 5).all()
    assert res.status[2] == 2 and res.selected[2] == -1 and np.isnan(res.theta[2]).all() and np.isnan(res.path[2]).all()
    assert np.isnan(res.cand_path[2]).all() and (res.status[:2] != 2).all()
    _check(gpu, "M200i", 5, cp, res, start, tp, ta, tref, _obstacles(), start_state=ss)
    # the same call without start_state uses every start inside the limits
    allin = cp.trace(start, tp, ta, tref, want_candidates=True)
    assert (allin.cand_status[2] != 5).all() and allin.status[2] != 2
    _check(gpu, "M200i", 5, cp, allin, start, tp, ta, tref, _obstacles())


def test_weights_and_the_outputs_without_candidates(gpu):
    lim, start, tp, ta, tref = _case(gpu, "M200i", 5, 3, 7, True, seed=31)
    robot = gpu.robotproperty2("M200i")
    w = np.array([5.0, 0.1, 1.0, 2.0, 0.3])
    cp = gpu.CartesianPath(robot, _obstacles(), steps=2, max_joint_step=0.4, weight=w)
    res = cp.trace(start, tp, ta, tref, want_candidates=True)
    _check(gpu, "M200i", 5, cp, res, start, tp, ta, tref, _obstacles())
    small = cp.trace(start, tp, ta, tref)                                    # the optional outputs NULL; path staged by the library
    assert not hasattr(small, "cand_path")
    for k in ("theta", "status", "path", "selected", "n_ok", "n_done", "clearance"):
        np.testing.assert_array_equal(getattr(small, k), getattr(res, k), err_msg=k)


def test_parity_with_the_cpu_restatement_in_axis_mode(gpu):
    P = CR.PARITY
    robot = gpu.robotproperty2(P["robot"])
    lim = robot.thetamax[:P["nj"]]
    arm, cases, movement, tol = CR.parity_case(lim)
    for c in cases:
        assert c.out.mean() <= 0.10
        cp = gpu.CartesianPath(robot, **c.kw)
        res = cp.trace(c.start, c.target_pos, c.target_axis, c.theta_ref, want_candidates=True)
        keep, ref = ~c.out, c.ref
        np.testing.assert_array_equal(res.cand_status[keep], ref.cand_status[keep])
        np.testing.assert_array_equal(res.cand_done[keep], ref.cand_done[keep])
        diff = np.nan_to_num(np.abs(res.cand_path - ref.cand_path), nan=0.0).max(axis=(2, 3))
        assert (np.isnan(res.cand_path) == np.isnan(ref.cand_path))[keep].all()
        print(f"[cart parity, reach {c.reach} m, K {c.kw['steps']}] {int(keep.sum())} candidates compared, left out {int(c.out.sum())} of {c.out.size}; "
              f"max |path - reference| {diff[keep].max():.2e} rad (CPU movement {movement:.2e}, tolerance {tol:.2e}); iterations equal on "
              f"{(res.cand_iter[keep] == ref.cand_iter[keep]).mean():.2f}")
        assert diff[keep].max() <= tol
        np.testing.assert_array_equal(res.cand_iter[keep], ref.cand_iter[keep])
        if keep.all():
            np.testing.assert_array_equal(res.selected, ref.selected)
            np.testing.assert_array_equal(res.status, ref.status)
            np.testing.assert_array_equal(res.n_done, ref.n_done)


def test_results_do_not_depend_on_the_batch_and_are_deterministic(gpu):
    import torch
    lim, start, tp, ta, tref = _case(gpu, "M200i", 5, 130, 64, True, seed=61)
    cp = gpu.CartesianPath(gpu.robotproperty2("M200i"), _obstacles(), steps=16)
    big = cp.trace(start, tp, ta, tref, want_candidates=True)
    again = cp.trace(start, tp, ta, tref, want_candidates=True)
    for k in NAMES:
        np.testing.assert_array_equal(getattr(big, k), getattr(again, k), err_msg=k)
    for rows in ([129], [5, 129, 64], [0]):                                  # alone, in a batch of 3 (other positions), first
        part = cp.trace(start[rows], tp[rows], ta[rows], tref[rows], want_candidates=True)
        for k in NAMES:
            np.testing.assert_array_equal(getattr(part, k), getattr(big, k)[rows], err_msg=k)
    # device tensors on a side stream behind other work, no host synchronisation in between; with and without the candidates
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    d = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    sd, tpd, tad, trd = d(start), d(tp), d(ta), d(tref)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        busy = torch.ones(2048, 2048, dtype=torch.float64, device=dev)
        for _ in range(4):
            busy = busy @ busy * 1e-4
        got = cp.trace_device(sd, tpd, tad, trd, want_candidates=True, stream=side)
        lean = cp.trace_device(sd, tpd, tad, trd, stream=side)
    side.synchronize()
    for k in NAMES:
        np.testing.assert_array_equal(getattr(got, k).cpu().numpy(), getattr(big, k), err_msg=k)
    for k in NAMES[:7]:
        np.testing.assert_array_equal(getattr(lean, k).cpu().numpy(), getattr(big, k), err_msg=k)


def test_plan_to_pose_with_an_approach(gpu, O):
    import torch
    pobs, s, g, region_g, region_s, off = gpu.RRTstar_problem()
    S = 8
    planner = gpu.RRTCFSPlanner(pobs, s, region_g, region_s, off, num_seed=2, max_slots=S)
    lim = s.robot.thetamax[:5]
    rng = np.random.default_rng(71)
    goals = []
    obs6, D = gpu.obs_to_array(pobs), np.array([o["D"] for o in pobs])
    while len(goals) < S:                                                    # grasp configurations that RRT's feasible() accepts
        gq = np.asarray(s.goal_th) + 0.15 * (2 * rng.random(5) - 1)
        d, _ = gpu.dist_arm(s.robot, gq[None], obs6)
        if ((d[0] - D) >= 0.02).all() and (gq > lim[:, 0]).all() and (gq < lim[:, 1]).all():
            goals.append(gq)
    tp, ta = gpu.tool_pose(s.robot, np.array(goals))
    x0 = np.broadcast_to(np.asarray(s.x0, float), (S, 5)).copy()
    dev = planner.device
    t64 = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    lines = [dict(l=o["l"], D=o["D"]) for o in pobs]

    def same(a, b, keys):
        for k in keys:
            x, y = getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), k
    # approach=None: today's composition (one IK launch, then plan) bit for bit, and none of the new fields
    res0 = planner.plan_to_pose(x0, tp, ta, seed=3)
    ik = gpu.IKSolver(s.robot, lines, njoint=5, device=dev)
    sol0 = ik.solve_device(t64(tp), t64(ta), t64(x0), seed=3)
    assert (sol0.status == 0).all()
    ref0 = planner.plan(x0, sol0.theta, 3)
    keys = [k for k, v in vars(ref0).items() if isinstance(v, torch.Tensor)]
    same(res0, ref0, keys)
    assert torch.equal(res0.goal, sol0.theta) and not hasattr(res0, "approach_path") and not hasattr(res0, "grasp")
    # approach: goal is the manual composition (IK at the pre-grasp with its candidates, then the trace from all of them)
    back, K = 0.05, 8
    res = planner.plan_to_pose(x0, tp, ta, seed=3, approach=back, approach_steps=K)
    un = ta / np.linalg.norm(ta, axis=1, keepdims=True)
    sol = ik.solve_device(t64(tp - back * un), t64(ta), t64(x0), seed=3, want_candidates=True)
    cart = gpu.CartesianPath(s.robot, lines, njoint=5, device=dev, steps=K)
    tr = cart.trace_device(sol.cand_theta, t64(tp), t64(ta), t64(x0), start_state=sol.cand_status, want_candidates=True)
    torch.cuda.synchronize()
    for a, b in ((res.goal, tr.theta), (res.approach_path, tr.path), (res.approach_status, tr.status), (res.approach_clearance, tr.clearance),
                 (res.grasp, tr.path[:, K]), (res.ik_status, sol.status), (res.ik_goal, sol.theta), (res.approach_selected, tr.selected)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=a.dtype.is_floating_point)
    ok = (tr.status == 0).cpu().numpy()
    ik_ok = (sol.status == 0).cpu().numpy()
    assert ik_ok.all() and ok.any()
    print(f"[cart planner] approach {back} m: {int(ok.sum())}/{S} slots with a line, {int((tr.selected == sol.selected).sum())} kept IK's own winner")
    # where IK's own winner completes its line, it stays the goal exactly
    own = tr.cand_status.gather(1, sol.selected.clamp(min=0).long()[:, None])[:, 0] == 0
    assert torch.equal(res.goal[own], sol.theta[own]) and torch.equal(tr.selected[own], sol.selected[own])
    # the grasp reaches the target with the tool on its axis, and every slot was planned to its goal
    gp, ga = gpu.tool_pose(s.robot, res.grasp[ok].cpu().numpy())
    assert np.linalg.norm(gp - tp[ok], axis=1).max() <= 1e-6 + 1e-12 and np.linalg.norm(ga - un[ok], axis=1).max() <= 1e-6 + 1e-12
    pp, _ = gpu.tool_pose(s.robot, res.goal[ok].cpu().numpy())
    assert np.abs(np.linalg.norm(pp - tp[ok], axis=1) - back).max() <= 2e-6   # IK's tolerance at the pre-grasp
    ref = planner.plan(x0, torch.where(tr.status[:, None] == 0, tr.theta, t64(x0)), 3)
    rows = torch.nonzero(tr.status == 0)[:, 0]
    for k in keys:
        x, y = getattr(res, k)[rows].cpu().numpy(), getattr(ref, k)[rows].cpu().numpy()
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), k
    bad = ~ok
    assert (res.status[bad] == -3).all() and (res.has_solution[bad] == 0).all() and (res.selected[bad] == -1).all()
    # no joint may move: every slot's IK solves and no approach exists -> every slot is masked with -3
    none = planner.plan_to_pose(x0, tp, ta, seed=3, approach=back, approach_steps=K, approach_options=dict(max_joint_step=1e-5))
    assert (none.ik_status == 0).all() and (none.approach_status == 1).all() and (none.status == -3).all()
    assert (none.has_solution == 0).all() and (none.selected == -1).all() and torch.isnan(none.goal).all() and torch.isnan(none.grasp).all()
    planner.close()
