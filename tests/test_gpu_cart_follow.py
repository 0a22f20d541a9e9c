"""Tool paths on the GPU (cfs_cart_follow*, CartesianPath.follow / follow_device, RRTCFSPlanner.plan_to_path) against cfs_tool_pose,
cfs_dist_arm, the selection rule restated in numpy, the CPU restatement tests/cart_follow_reference.py, the straight line of
trace_device and, for meshes, tests/cart_mesh_reference.apply_meshes on the device's own line-only answer.

Shapes: T = 1, 3, 130 (33 workgroups, the last one ragged); R = 64, 7, 1 (idle lanes); (M, K) = (2, 16), (3, 4) and (5, 1) (the dense
table: four segment boundaries, every row a pose of the table).  M200i (5 joints) with two line obstacles, M16iB (6) and 2L (2), with and
without the axis (the 2L position only).  A target's polyline passes the tool poses of configurations near the first candidate of its
row, so the paths are short and reachable; the other candidates are configurations near that one and, every fifth, a random one far
away.  The independent properties are checked for every candidate through cand_path."""
import numpy as np
import pytest

import cart_follow_reference as FR
import cart_mesh_reference as CM
import cart_reference as CR
import ik_mesh_reference as K
import ik_reference as R
import rrt_mesh_reference as M
from test_gpu_cart import _obstacles

pytestmark = pytest.mark.gpu

TOL = 1e-6
ROBOTS = [("M200i", 5, True), ("M200i", 5, False), ("M16iB", 6, True), ("M16iB", 6, False), ("2L", 2, False)]
NAMES = ("theta", "status", "path", "selected", "n_ok", "n_done", "clearance", "cand_status", "cand_done", "cand_iter", "cand_end", "cand_path")


def _case(pkg, name, nj, T, Rn, Mp, axis, seed, reach=0.1):
    """starts (T, R, nj), path_pos (T, M, 3), path_axis | None, theta_ref: pose 0 is the pose of candidate 0, pose j the pose of a
    configuration `reach` rad (per joint, at most) from the one before it"""
    robot = pkg.robotproperty2(name)
    lim = robot.thetamax[:nj]
    rng = np.random.default_rng(seed)
    q = R.in_limit_configs(lim, T, seed, shrink=0.6)
    start = q[:, None, :] + 0.03 * rng.standard_normal((T, Rn, nj))
    start[:, 0] = q
    far = R.in_limit_configs(lim, T * Rn, seed + 1, shrink=0.9).reshape(T, Rn, nj)
    start[:, 4::5] = far[:, 4::5]
    start = np.clip(start, lim[:, 0], lim[:, 1])
    way = np.zeros((T, Mp, nj))
    way[:, 0] = q
    for j in range(1, Mp):
        way[:, j] = np.clip(way[:, j - 1] + reach * (2 * rng.random((T, nj)) - 1), lim[:, 0], lim[:, 1])
    pp, pa = pkg.tool_pose(robot, way.reshape(-1, nj), njoint=nj)
    tref = R.in_limit_configs(lim, T, seed + 2, shrink=0.6)
    return lim, start, pp.reshape(T, Mp, 3), (pa.reshape(T, Mp, 3) if axis else None), tref


def _rows(pos, axs, Ks):
    """(T, N, 3) points and axes (None in position-only mode) of every target's polyline, restated from the header"""
    both = [FR.rows_of(pos[t], None if axs is None else FR.unit_rows(axs[t]), Ks) for t in range(pos.shape[0])]
    return np.stack([b[0] for b in both]), (None if axs is None else np.stack([b[1] for b in both]))


def _check(pkg, name, nj, cp, res, start, pos, axs, tref, obs, start_state=None):
    """the independent properties of every candidate, the reasons of the failed ones, the winner's rows and the selection"""
    with np.errstate(invalid="ignore", divide="ignore"):                    # rows without a start have no path
        _check_body(pkg, name, nj, cp, res, start, pos, axs, tref, obs, start_state)


def _check_body(pkg, name, nj, cp, res, start, pos, axs, tref, obs, start_state):
    robot = pkg.robotproperty2(name)
    T, Rn, N, _ = res.cand_path.shape
    assert N == (pos.shape[1] - 1) * cp.steps + 1
    st, done, path = res.cand_status, res.cand_done, res.cand_path
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
    # which rows hold configurations: theta_0..theta_done of a candidate with an accepted row 0, NaN elsewhere
    have = ~np.isnan(path).any(axis=3)
    assert (have == ~np.isnan(path).all(axis=3)).all()
    row0 = have[:, :, 0]
    assert (have == (row0[:, :, None] & (np.arange(N)[None, None, :] <= done[:, :, None]))).all()
    assert ((st == 0) == (row0 & (done == N - 1))).all() and (done[~row0] == 0).all()
    # no start: exactly the starts the contract refuses
    inside = np.isfinite(start).all(axis=2) & (np.nan_to_num(start) >= lo).all(axis=2) & (np.nan_to_num(start) <= hi).all(axis=2)
    usable = inside if start_state is None else inside & (start_state == 0)
    assert ((st == 5) == ~usable).all()
    assert np.isnan(res.cand_end[st == 5]).all() and (res.cand_iter[st == 5] == 0).all()
    # every accepted configuration: on its polyline point, inside the limits, free; every row jump-bounded, row 0 against the start
    pk, ak = _rows(pos, axs, cp.steps)
    pk = np.broadcast_to(pk[:, None], (T, Rn, N, 3))
    ak = None if ak is None else np.broadcast_to(ak[:, None], (T, Rn, N, 3))
    flat = path[have]
    p, dr = poses(flat)
    assert np.linalg.norm(p - pk[have], axis=1).max(initial=0.0) <= cp.tol_pos + 1e-12
    if ak is not None:
        assert np.linalg.norm(dr - ak[have], axis=1).max(initial=0.0) <= cp.tol_axis + 1e-12
    assert (flat >= lo).all() and (flat <= hi).all()
    cl = np.full((T, Rn, N), np.inf)
    cl[have] = clearance(flat)
    assert cl.min() >= -1e-12
    chain = np.concatenate([start[:, :, None, :], path], axis=2)            # the start, then the rows
    step = np.abs(np.diff(chain, axis=2)).max(axis=3)
    assert (step[have] <= cp.max_joint_step).all()
    # a start that already solves the first pose: row 0 is the start bit for bit
    p0, d0 = poses(start[row0])
    on0 = np.linalg.norm(p0 - pk[:, :, 0][row0], axis=1) <= cp.tol_pos * 0.5
    if ak is not None:
        on0 &= np.linalg.norm(d0 - ak[:, :, 0][row0], axis=1) <= cp.tol_axis * 0.5
    np.testing.assert_array_equal(path[:, :, 0][row0][on0], start[row0][on0])
    # the stated reason holds at cand_end; `before` is the configuration the failing row started from, nxt that row
    end = res.cand_end
    last = np.take_along_axis(path, done[:, :, None, None].repeat(nj, 3), axis=2)[:, :, 0]     # theta_done
    before = np.where(row0[:, :, None], last, start)
    nxt = np.where(row0, np.minimum(done + 1, N - 1), 0)
    want_p = np.take_along_axis(pk, nxt[:, :, None, None].repeat(3, 3), axis=2)[:, :, 0]
    np.testing.assert_array_equal(end[st == 0], path[:, :, N - 1][st == 0])
    m = st == 2
    assert (clearance(end[m]) < 1e-12).all()
    m = st == 4
    assert (np.abs(end[m] - before[m]).max(axis=1) > cp.max_joint_step).all()
    for m in (st == 2, st == 4):                                            # these ended ON the next polyline point
        pe, de = poses(end[m])
        assert m.sum() == 0 or np.linalg.norm(pe - want_p[m], axis=1).max() <= cp.tol_pos + 1e-12
    m = st == 1
    if m.any():
        pe, de = poses(end[m])
        ep = np.linalg.norm(pe - want_p[m], axis=1)
        ea = np.zeros_like(ep) if ak is None else np.linalg.norm(de - np.take_along_axis(ak, nxt[:, :, None, None].repeat(3, 3), axis=2)[:, :, 0][m], axis=1)
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
        np.testing.assert_array_equal(res.theta[t], start[t, r])           # the winner's START, not row 0
        np.testing.assert_array_equal(res.path[t], path[t, r])
        if obs6 is None:
            assert np.isposinf(res.clearance[t])
        else:
            assert abs(res.clearance[t] - cl[t, r].min()) <= 1e-12 and res.clearance[t] >= 0


@pytest.mark.parametrize("name,nj,axis", ROBOTS)
@pytest.mark.parametrize("T,Rn,Mp,Ks", [(1, 64, 2, 16), (3, 7, 3, 4), (130, 1, 5, 1), (130, 64, 3, 4), (3, 64, 5, 1), (1, 7, 2, 16)])
def test_every_candidate_keeps_the_contract(gpu, name, nj, axis, T, Rn, Mp, Ks):
    lim, start, pos, axs, tref = _case(gpu, name, nj, T, Rn, Mp, axis, seed=200 + T + Rn + Mp)
    obs = _obstacles() if name == "M200i" else None
    cp = gpu.CartesianPath(gpu.robotproperty2(name), obs, steps=Ks, max_joint_step=0.2 if Ks > 2 else 0.4)
    res = cp.follow(start, pos, axs, tref, want_candidates=True)
    st = res.cand_status
    print(f"[follow {name} axis={axis} T={T} R={Rn} M={Mp} K={Ks}] solved {int((res.status == 0).sum())}/{T}, candidate states 0..5 "
          f"{[int((st == s).sum()) for s in range(6)]}, largest cand_iter {int(res.cand_iter.max())}")
    _check(gpu, name, nj, cp, res, start, pos, axs, tref, obs)
    assert (st != 3).all()
    if nj >= 5:                                                              # the short path from the configuration on the first pose;
        assert (st[:, 0] == 0).mean() >= 0.5                                 # the 2L's tool moves on a surface that holds no straight chord
    elif Ks > 1:
        assert (st == 1).any()


def _ell(gpu, q, reach, side):
    """the L-shaped polylines of the parity case (tests/cart_follow_reference.py) for configurations q of the M200i"""
    p, a = gpu.tool_pose(gpu.robotproperty2("M200i"), q)
    e = np.cross(a, [0.0, 0.0, 1.0])
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    return np.stack([p, p + reach * a, p + reach * a + side * e], axis=1), np.stack([a, a, a], axis=1)


def test_collision_on_the_second_segment(gpu, O):
    """a line obstacle laid across the SECOND segment: state 2 at the row the restatement names, after a segment boundary"""
    robot = gpu.robotproperty2("M200i")
    lim = robot.thetamax[:5]
    arm = R.Arm(O.robotproperty2("M200i"), 5)
    q = R.in_limit_configs(lim, 6, 17, shrink=0.5)
    Ks, reach, side, found = 4, 0.05, 0.2, 0
    pos, axs = _ell(gpu, q, reach, side)
    for i, x in enumerate(q):
        a, e = axs[i, 0], (pos[i, 2] - pos[i, 1]) / side
        # across the second segment, 15 cm from its first point along e, parallel to the tool axis: the tool point clears the 4 cm
        # margin by 11 cm at row K and loses 5 cm per row, so rows K+1 and K+2 are free (6 cm, 1 cm) and row K+3 is 4 cm inside
        mid = pos[i, 1] + 0.15 * e
        obs = [dict(l=np.stack([mid - 0.5 * a, mid + 0.5 * a], axis=1), D=0.04)]
        o6, Dm = gpu.obs_to_array(obs), np.array([0.04])
        kw = dict(steps=Ks, max_iter=20, max_joint_step=0.3, tol_pos=TOL, tol_axis=TOL)
        ref = FR.follow(arm, x[None, None], pos[i][None], axs[i][None], x, lim[:, 0], lim[:, 1], obs=o6, D=Dm, **kw)
        if ref.cand_status[0, 0] != 2 or ref.cand_done[0, 0] < Ks:
            continue                                                         # this configuration does not make the case
        # the deciding clearances are far from zero, so rounding cannot move the row
        before, after = arm.clearance(ref.cand_path[0, 0, ref.cand_done[0, 0]], o6, Dm), arm.clearance(ref.cand_end[0, 0], o6, Dm)
        if not (before > 1e-6 and after < -1e-6):
            continue
        found += 1
        cp = gpu.CartesianPath(robot, obs, steps=Ks, max_joint_step=0.3)
        res = cp.follow(x[None, None], pos[i], axs[i], x, want_candidates=True)
        assert res.cand_status[0, 0] == 2 and res.status[0] == 1 and res.selected[0] == -1 and res.n_ok[0] == 0
        assert res.cand_done[0, 0] == ref.cand_done[0, 0] >= Ks and res.n_done[0] == ref.cand_done[0, 0]
        _check(gpu, "M200i", 5, cp, res, x[None, None], pos[i][None], axs[i][None], x[None], obs)
        free = gpu.CartesianPath(robot, steps=Ks, max_joint_step=0.3).follow(x[None, None], pos[i], axs[i], x, want_candidates=True)
        # without the obstacle the colliding row is accepted (bit for bit the configuration that collided)
        np.testing.assert_array_equal(free.cand_path[0, 0, ref.cand_done[0, 0] + 1], res.cand_end[0, 0])
        assert free.cand_status[0, 0] != 2 and (free.status[0] != 0 or np.isposinf(free.clearance[0]))
    assert found >= 2


def test_out_of_reach_on_the_second_segment_and_a_joint_jump_at_row_0(gpu):
    robot = gpu.robotproperty2("M200i")
    lim, start, pos, axs, tref = _case(gpu, "M200i", 5, 3, 7, 3, True, seed=23)
    start[:, 4] = start[:, 3]                                                # no far candidate
    reach = sum(np.hypot(robot.DH[j, 2], robot.DH[j, 1]) for j in range(5)) + 1.0
    far = pos.copy()
    far[:, 2] = robot.base + np.array([reach, 0.0, 0.0])
    Ks = 2
    cp = gpu.CartesianPath(robot, steps=Ks, max_joint_step=100.0)            # no jump can end a candidate first
    res = cp.follow(start, far, axs, tref, want_candidates=True)
    assert (res.cand_status == 1).all() and (res.cand_done < 2 * Ks).all()
    assert (res.cand_done[:, 0] >= Ks).all()                                 # the candidate on the first pose follows the first segment
    assert (res.status == 1).all() and (res.n_ok == 0).all() and (res.selected == -1).all() and np.isnan(res.theta).all() and np.isnan(res.path).all()
    _check(gpu, "M200i", 5, cp, res, start, far, axs, tref, None)
    # row 0 is tested against the start: starts 0.03 rad from the solution of the first pose jump under a bound of 1e-4 rad; the
    # start ON the first pose passes row 0 and jumps at row 1
    cj = gpu.CartesianPath(robot, steps=Ks, max_joint_step=1e-4)
    jump = cj.follow(start, pos, axs, tref, want_candidates=True)
    assert (jump.cand_status == 4).all() and (jump.cand_done == 0).all() and (jump.status == 1).all() and (jump.n_done == 0).all()
    assert np.isnan(jump.cand_path[:, 1:]).all() and not np.isnan(jump.cand_path[:, 0, 0]).any() and np.isnan(jump.cand_path[:, 0, 1:]).all()
    np.testing.assert_array_equal(jump.cand_path[:, 0, 0], start[:, 0])
    _check(gpu, "M200i", 5, cj, jump, start, pos, axs, tref, None)
    # a start far from the first pose, under the usual bound
    lim2 = robot.thetamax[:5]
    away = R.in_limit_configs(lim2, 21, 24, shrink=0.9).reshape(3, 7, 5)
    cf = gpu.CartesianPath(robot, steps=Ks, max_joint_step=0.2)
    res = cf.follow(away, pos, axs, tref, want_candidates=True)
    assert ((res.cand_status == 4) & (res.cand_done == 0) & np.isnan(res.cand_path[:, :, 0, 0])).any()
    _check(gpu, "M200i", 5, cf, res, away, pos, axs, tref, None)


def test_no_start(gpu):
    lim, start, pos, axs, tref = _case(gpu, "M200i", 5, 3, 7, 3, True, seed=29)
    robot = gpu.robotproperty2("M200i")
    ss = np.zeros((3, 7), np.int32)
    ss[0, 1], ss[0, 2], ss[0, 3] = 1, 2, 3                                   # IK's states of restarts that did not end free
    start[0, 5, 2] = lim[2, 1] + 1e-9                                        # outside by a hair
    start[0, 6, 0] = np.nan
    start[1, 0, 4] = np.inf
    ss[2, :] = 1                                                             # a target without any start
    cp = gpu.CartesianPath(robot, _obstacles(), steps=2, max_joint_step=0.4)
    res = cp.follow(start, pos, axs, tref, start_state=ss, want_candidates=True)
    assert (res.cand_status[0, [1, 2, 3, 5, 6]] == 5).all() and res.cand_status[1, 0] == 5 and (res.cand_status[2] == 5).all()
    assert res.status[2] == 2 and res.selected[2] == -1 and np.isnan(res.theta[2]).all() and np.isnan(res.path[2]).all()
    assert np.isnan(res.cand_path[2]).all() and (res.status[:2] != 2).all()
    _check(gpu, "M200i", 5, cp, res, start, pos, axs, tref, _obstacles(), start_state=ss)
    allin = cp.follow(start, pos, axs, tref, want_candidates=True)           # without start_state every start inside the limits is used
    assert (allin.cand_status[2] != 5).all() and allin.status[2] != 2
    _check(gpu, "M200i", 5, cp, allin, start, pos, axs, tref, _obstacles())


def test_weights_the_outputs_without_candidates_and_the_device_entrys_workspace(gpu):
    import ctypes as C
    import torch
    from motionplanning_5d_m_amd import _lib
    lim, start, pos, axs, tref = _case(gpu, "M200i", 5, 3, 7, 3, True, seed=31)
    robot = gpu.robotproperty2("M200i")
    w = np.array([5.0, 0.1, 1.0, 2.0, 0.3])
    cp = gpu.CartesianPath(robot, _obstacles(), steps=2, max_joint_step=0.4, weight=w)
    res = cp.follow(start, pos, axs, tref, want_candidates=True)
    _check(gpu, "M200i", 5, cp, res, start, pos, axs, tref, _obstacles())
    small = cp.follow(start, pos, axs, tref)                                 # the optional outputs NULL; path staged by the library
    assert not hasattr(small, "cand_path")
    for k in NAMES[:7]:
        np.testing.assert_array_equal(getattr(small, k), getattr(res, k), err_msg=k)
    # the device entry refuses `path` without `cand_path` and writes nothing
    dev = torch.device("cuda", 0)
    d64 = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    sd, pd, ad, td = d64(start), d64(pos), d64(axs), d64(tref)
    _, obs_d, D_d = cp._on(dev, None)
    theta, status, path = torch.full((3, 5), 7.0, dtype=torch.float64, device=dev), torch.full((3,), 7, dtype=torch.int32, device=dev), \
        torch.full((3, 5, 5), 7.0, dtype=torch.float64, device=dev)
    o = _lib.cfs_cart_out()
    o.theta, o.status, o.path = theta.data_ptr(), status.data_ptr(), path.data_ptr()
    d = cp._desc(True, 7, obs_d, D_d)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = _lib.lib().cfs_cart_follow_device(C.byref(d), 3, 3, p(sd), None, p(pd), p(ad), p(td), C.byref(o), None)
    assert rc == -1 and b"cand_path" in _lib.lib().cfs_last_error()
    torch.cuda.synchronize()
    assert (theta == 7.0).all() and (status == 7).all() and (path == 7.0).all()


def test_parity_with_the_cpu_restatement_in_axis_mode(gpu):
    P = FR.PARITY
    robot = gpu.robotproperty2(P["robot"])
    lim = robot.thetamax[:P["nj"]]
    arm, cases, movement, tol = FR.parity_case(lim)
    for c in cases:
        assert c.out.mean() <= 0.10
        cp = gpu.CartesianPath(robot, **c.kw)
        res = cp.follow(c.start, c.path_pos, c.path_axis, c.theta_ref, want_candidates=True)
        keep, ref = ~c.out, c.ref
        diff = np.nan_to_num(np.abs(res.cand_path - ref.cand_path), nan=0.0).max(axis=(2, 3))
        print(f"[follow parity, reach {c.reach} m, side {c.side} m, K {c.kw['steps']}] {int(keep.sum())} candidates compared, left out "
              f"{int(c.out.sum())} of {c.out.size}; states equal on {(res.cand_status[keep] == ref.cand_status[keep]).mean():.2f}, max |path - reference| "
              f"{diff[keep].max():.2e} rad (CPU movement {movement:.2e}, tolerance {tol:.2e}); iterations equal on "
              f"{(res.cand_iter[keep] == ref.cand_iter[keep]).mean():.2f}")
        np.testing.assert_array_equal(res.cand_status[keep], ref.cand_status[keep])
        np.testing.assert_array_equal(res.cand_done[keep], ref.cand_done[keep])
        assert (np.isnan(res.cand_path) == np.isnan(ref.cand_path))[keep].all()
        assert diff[keep].max() <= tol
        np.testing.assert_array_equal(res.cand_iter[keep], ref.cand_iter[keep])
        if keep.all():
            np.testing.assert_array_equal(res.selected, ref.selected)
            np.testing.assert_array_equal(res.status, ref.status)
            np.testing.assert_array_equal(res.n_done, ref.n_done)


def test_a_two_pose_path_from_the_starts_own_pose_is_trace_device(gpu):
    """reduction to the straight line on the device: section 23's parity case, one candidate per launch row (R = 1), the path
    [cfs_tool_pose(start), target]"""
    import torch
    P = CR.PARITY
    robot = gpu.robotproperty2(P["robot"])
    lim = robot.thetamax[:P["nj"]]
    arm, cases, _, _ = CR.parity_case(lim)
    _, _, movement, tol = FR.parity_case(lim)
    dev = torch.device("cuda", 0)
    d64 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
    for c in cases:
        T, Rn, nj = c.start.shape
        s = c.start.reshape(T * Rn, 1, nj)
        tp, ta, tr = np.repeat(c.target_pos, Rn, axis=0), np.repeat(c.target_axis, Rn, axis=0), np.repeat(c.theta_ref, Rn, axis=0)
        p0, a0 = gpu.tool_pose(robot, s[:, 0])
        cp = gpu.CartesianPath(robot, **c.kw)
        line = cp.trace_device(d64(s), d64(tp), d64(ta), d64(tr), want_candidates=True)
        got = cp.follow_device(d64(s), d64(np.stack([p0, tp], axis=1)), d64(np.stack([a0, ta], axis=1)), d64(tr), want_candidates=True)
        torch.cuda.synchronize()
        keep = ~c.out.reshape(-1)
        n = lambda x: x.cpu().numpy()[:, 0][keep]  # noqa: E731
        diff = np.nan_to_num(np.abs(n(got.cand_path) - n(line.cand_path)), nan=0.0).max()
        print(f"[follow vs trace_device, reach {c.reach} m, K {c.kw['steps']}] {int(keep.sum())} candidates, max |path - trace| {diff:.2e} rad "
              f"(tolerance {tol:.2e})")
        for k in ("cand_status", "cand_done", "cand_iter"):
            np.testing.assert_array_equal(n(getattr(got, k)), n(getattr(line, k)), err_msg=k)
        assert (np.isnan(n(got.cand_path)) == np.isnan(n(line.cand_path))).all() and diff <= tol


# ---- meshes ----------------------------------------------------------------------------------------------------------------------------
VARIANTS = ["per_lane", "wave", "small_frontier"]
CAND = ("cand_status", "cand_done", "cand_iter", "cand_end", "cand_path")
TARGET = ("theta", "status", "path", "selected", "n_ok", "n_done")


def test_meshes_on_an_l_shaped_path_past_the_cylinder(gpu, O):
    """cfs_cart_follow_mesh on the cylinder scene of cart_mesh_reference: the first segment is the scene's own approach, the second
    one leads 0.2 m towards the cylinder's axis (on the CPU restatement: 40 candidates rejected at row 7, three rows past the boundary).  Against apply_meshes on the device's own line-only answer (rules 1-6 with K+1 = N);
    the three flag settings bit-identical; a mesh no row comes near changes nothing."""
    arm, lim, lines, tri, inp = CM.scene()
    ids = CM.mesh_ids()
    robot = gpu.robotproperty2("M200i")
    ik = gpu.IKSolver(robot, lines, restarts=64, max_iter=inp.ik_max_iter, tol_pos=inp.tol_pos, tol_axis=inp.tol_axis)
    sol = ik.solve(inp.pre_pos, inp.pre_axis, inp.theta_ref, seed=CM.SEED, want_candidates=True)
    centre = np.asarray(tri, float).reshape(-1, 3).mean(axis=0)
    to = centre[None, :] - inp.target_pos
    to[:, 2] = 0.0
    to /= np.linalg.norm(to, axis=1, keepdims=True)
    pos = np.stack([inp.pre_pos, inp.target_pos, inp.target_pos + 0.2 * to], axis=1)
    axs = np.stack([inp.pre_axis] * 3, axis=1)
    Ks = 4
    args = (sol.cand_theta, pos, axs, inp.theta_ref)
    kw = dict(start_state=sol.cand_status, want_candidates=True)
    mesh = gpu.Mesh(tri=tri)
    line = gpu.CartesianPath(robot, lines, steps=Ks, **CM.CART).follow(*args, **kw)
    res = {}
    for v in [None] + VARIANTS:
        res[v] = gpu.CartesianPath(robot, lines + [dict(mesh=mesh, D=M.CYL_D)], steps=Ks, meshes=True, mesh_variant=v, **CM.CART).follow(*args, **kw)
    got = res[None]
    want = CM.apply_meshes(O, O.robotproperty2("M200i"), line, sol.cand_theta, inp.theta_ref, ids)
    np.testing.assert_array_equal(got.cand_iter, line.cand_iter)
    near = want.cand_closest < CM.MARGIN                                      # test_gpu_cart_mesh.py's rule: within rounding of a threshold
    second = (want.cand_m > Ks).sum()
    print(f"[follow mesh] candidates with rows {int((~np.isnan(line.cand_path[:, :, 0, 0])).sum())}, rejected {int((want.cand_m >= 0).sum())} "
          f"({int(second)} on the second segment), closest call {want.cand_closest.min():.2e} m, status {got.status.tolist()} line-only {line.status.tolist()}")
    assert not near.any() and second > 0
    for k in CAND + TARGET:
        np.testing.assert_array_equal(getattr(got, k), getattr(want, k), err_msg=k)
    first = np.where(np.isnan(got.cand_path[:, :, :, 0]).any(axis=2), np.isnan(got.cand_path[:, :, :, 0]).argmax(axis=2), -1)
    hit = want.cand_m >= 0
    np.testing.assert_array_equal(first[hit], want.cand_m[hit])              # the first rejected row
    for v in VARIANTS:
        for k in NAMES:
            np.testing.assert_array_equal(getattr(res[v], k), getattr(got, k), err_msg=f"{v}: {k}")
    # a mesh no row comes near: the line-only outputs bit for bit (the clearance too: the far mesh is farther than every line)
    away = gpu.Mesh(tri=np.asarray(tri, float) + np.array([0.0, 0.0, 50.0]))
    same = gpu.CartesianPath(robot, lines + [dict(mesh=away, D=M.CYL_D)], steps=Ks, meshes=True, **CM.CART).follow(*args, **kw)
    for k in NAMES:
        np.testing.assert_array_equal(getattr(same, k), getattr(line, k), err_msg=f"far mesh: {k}")


# ---- batch independence and determinism ----------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_batch_and_are_deterministic(gpu):
    import torch
    lim, start, pos, axs, tref = _case(gpu, "M200i", 5, 130, 64, 3, True, seed=61)
    cp = gpu.CartesianPath(gpu.robotproperty2("M200i"), _obstacles(), steps=4)
    big = cp.follow(start, pos, axs, tref, want_candidates=True)
    again = cp.follow(start, pos, axs, tref, want_candidates=True)
    for k in NAMES:
        np.testing.assert_array_equal(getattr(big, k), getattr(again, k), err_msg=k)
    for rows in ([129], [5, 129, 64], [0]):                                  # alone, in a batch of 3 (other positions), first
        part = cp.follow(start[rows], pos[rows], axs[rows], tref[rows], want_candidates=True)
        for k in NAMES:
            np.testing.assert_array_equal(getattr(part, k), getattr(big, k)[rows], err_msg=k)
    # device tensors on a side stream behind other work, no host synchronisation in between; with and without the candidates
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    d = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    sd, pd, ad, trd = d(start), d(pos), d(axs), d(tref)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        busy = torch.ones(2048, 2048, dtype=torch.float64, device=dev)
        for _ in range(4):
            busy = busy @ busy * 1e-4
        got = cp.follow_device(sd, pd, ad, trd, want_candidates=True, stream=side)
        lean = cp.follow_device(sd, pd, ad, trd, stream=side)
    side.synchronize()
    for k in NAMES:
        np.testing.assert_array_equal(getattr(got, k).cpu().numpy(), getattr(big, k), err_msg=k)
    for k in NAMES[:7]:
        np.testing.assert_array_equal(getattr(lean, k).cpu().numpy(), getattr(big, k), err_msg=k)


# ---- the planner -----------------------------------------------------------------------------------------------------------------------
def test_plan_to_path(gpu):
    import torch
    pobs, s, g, region_g, region_s, off = gpu.RRTstar_problem()
    S, Ks = 4, 4
    planner = gpu.RRTCFSPlanner(pobs, s, region_g, region_s, off, num_seed=2, max_slots=S)
    lim = s.robot.thetamax[:5]
    rng = np.random.default_rng(71)
    goals = []
    obs6, D = gpu.obs_to_array(pobs), np.array([o["D"] for o in pobs])
    while len(goals) < S:                                                    # first configurations that RRT's feasible() accepts
        gq = np.asarray(s.goal_th) + 0.15 * (2 * rng.random(5) - 1)
        d, _ = gpu.dist_arm(s.robot, gq[None], obs6)
        if ((d[0] - D) >= 0.02).all() and (gq > lim[:, 0]).all() and (gq < lim[:, 1]).all():
            goals.append(gq)
    pos, axs = _ell(gpu, np.array(goals), 0.04, 0.04)
    x0 = np.broadcast_to(np.asarray(s.x0, float), (S, 5)).copy()
    dev = planner.device
    t64 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)  # noqa: E731
    lines = [dict(l=o["l"], D=o["D"]) for o in pobs]
    res = planner.plan_to_path(x0, pos, axs, seed=3, path_steps=Ks)
    # the manual composition: IK at the first pose with its candidates, follow_device from all of them, plan() to the winners' row 0
    ik = gpu.IKSolver(s.robot, lines, njoint=5, device=dev)
    sol = ik.solve_device(t64(pos[:, 0]), t64(axs[:, 0]), t64(x0), seed=3, want_candidates=True)
    cart = gpu.CartesianPath(s.robot, lines, njoint=5, device=dev, steps=Ks)
    fo = cart.follow_device(sol.cand_theta, t64(pos), t64(axs), t64(x0), start_state=sol.cand_status, want_candidates=True)
    torch.cuda.synchronize()
    for a, b in ((res.goal, fo.path[:, 0]), (res.tool_path, fo.path), (res.tool_path_status, fo.status), (res.tool_path_clearance, fo.clearance),
                 (res.tool_path_selected, fo.selected), (res.ik_status, sol.status), (res.ik_goal, sol.theta)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=a.dtype.is_floating_point)
    ok, ik_ok = (fo.status == 0).cpu().numpy(), (sol.status == 0).cpu().numpy()
    assert tuple(res.tool_path.shape) == (S, 2 * Ks + 1, 5) and ik_ok.all() and ok.any()
    print(f"[follow planner] {int(ok.sum())}/{S} slots with a path, {int((fo.selected == sol.selected).sum())} kept IK's own winner")
    # IK's candidates solve the first pose, so row 0 of a winner's path is its start
    assert torch.equal(res.goal[torch.as_tensor(ok, device=dev)], fo.theta[torch.as_tensor(ok, device=dev)])
    ref = planner.plan(x0, torch.where(fo.status[:, None] == 0, fo.path[:, 0], t64(x0)), 3)
    rows = torch.nonzero(fo.status == 0)[:, 0]
    for k, v in vars(ref).items():
        if isinstance(v, torch.Tensor):
            x, y = getattr(res, k)[rows].cpu().numpy(), v[rows].cpu().numpy()
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), k
    # -3: every slot's IK solves and no joint may move, so no candidate follows the path
    none = planner.plan_to_path(x0, pos, axs, seed=3, path_steps=Ks, path_options=dict(max_joint_step=1e-5))
    assert (none.ik_status == 0).all() and (none.tool_path_status == 1).all() and (none.status == -3).all()
    assert (none.has_solution == 0).all() and (none.selected == -1).all() and torch.isnan(none.goal).all() and torch.isnan(none.tool_path).all()
    # -2: a first pose out of reach has no IK solution; the other slots are planned as before
    out = pos.copy()
    out[1] += np.array([50.0, 0.0, 0.0])
    mixed = planner.plan_to_path(x0, out, axs, seed=3, path_steps=Ks)
    assert mixed.ik_status[1] != 0 and mixed.status[1] == -2 and mixed.has_solution[1] == 0 and mixed.selected[1] == -1
    assert mixed.tool_path_status[1] == 2 and torch.isnan(mixed.goal[1]).all()
    keep = [i for i in range(S) if i != 1]
    assert torch.equal(mixed.tool_path_status[keep], res.tool_path_status[keep])
    planner.close()
