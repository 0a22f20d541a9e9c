"""Path timing on the GPU (cfs_path_time*, PathTimer.time / time_device, the planner's path_timing) against the properties the contract
promises, checked on the device's own output with tests/path_time_reference.py's checkers, and against the CPU restatement.

Shapes: G = 1, 3, 130 (33 workgroups of the selection, the last one ragged; 8320 paths = 33 workgroups of the timing, the last one
ragged) x R = 64, 7, 1 x N = 3 (one interior row), 4, 17, 257 (the largest), all 36.  M200i (5 joints), M16iB (6) and 2L (2), with
and without a feed.  Paths are straight joint moves plus a sine term of at most 0.2 rad per row; every fifth path has a state != 0, path 1 a NaN
row and path 2 a repeated row (where the batch has that many).  The per-path properties are checked on the first 24 paths of a batch
and on its last, the batch-wide ones (statuses, NaN rows, the selection) on all."""
import functools

import numpy as np
import pytest

import path_time_reference as PT

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
ROBOTS = [("M200i", 5), ("M16iB", 6), ("2L", 2)]
SHAPES = [(G, R, N) for G in (1, 3, 130) for R in (64, 7, 1) for N in (3, 4, 17, 257)]
FEED = 0.25


def _limits(nj):
    return np.linspace(0.8, 1.6, nj), np.linspace(3.0, 1.5, nj)


@functools.lru_cache(maxsize=2)
def _inputs(pkg, name, nj, G, R, N, seed):
    """paths (G, R, N, nj), state (G, R), the expected status (G, R); made once for the cases that share them and left unchanged"""
    lim = pkg.robotproperty2(name).thetamax[:nj]
    paths = PT.smooth_paths(lim, G, R, N, seed)
    flat = paths.reshape(G * R, N, nj)
    state = np.zeros(G * R, np.int32)
    want = np.zeros(G * R, np.int32)
    state[4::5] = 3
    want[4::5] = 1
    if G * R >= 4:
        flat[1, N // 2, nj - 1] = np.nan
        flat[2, N - 1] = flat[2, N - 2]
        want[1], want[2] = 2, 4
    return paths, state.reshape(G, R), want.reshape(G, R)


def _points(pkg, name, nj, q):
    return pkg.tool_pose(pkg.robotproperty2(name), q.reshape(-1, nj), njoint=nj)[0].reshape(q.shape[:-1] + (3,))


def _check_path(q, time, sdot, duration, vmax, amax, feed, pts, k):
    """the properties of one timed path.  The acceleration and speed ratios are built from the rows and the device's sdot alone.  With
    a feed the tool points are cfs_tool_pose's, the kernel's own are not an output: the two evaluate the same expression with and
    without contraction and differ by a few roundings of |p|, 16 eps |p| at most per point, which moves a row's e_n by 32 eps |p|: an
    allowance fk_n = 32 eps |p| / e_n of that row alone on its feed ratio.  cap_n's feed term is (feed / e_n)^2 and moves by 2 fk_n; a
    budget moves by no more than its row's cap, relative (gamma = 0.5); row n's three candidates read cap_n and cap_{n-1}."""
    N = q.shape[0]
    T = PT.terms(q, vmax, amax, feed, pts, 0.5, k)
    stops = PT.stop_rows(N, k)
    assert (sdot[stops] == 0.0).all() and (sdot[~stops] > 0).all()
    assert time[0] == 0.0 and (np.diff(time) > 0).all() and duration == time[-1]
    acc, vel, _ = PT.limit_ratios(q, sdot, vmax, amax, feed, pts)
    assert acc <= 1.0 + 1e-12 and vel <= 1.0 + 1e-12, (acc, vel)
    fk = np.zeros(N)
    if T.e is not None:
        with np.errstate(divide="ignore"):
            fk = 32 * EPS * np.abs(pts).max() / T.e
        ratio = T.e * sdot / feed
        assert (ratio <= 1.0 + 1e-12 + fk).all(), float((ratio - fk).max())
    # no slack: sdot^2 is b to 3 roundings, and so are the two neighbours' in the candidates
    near = np.maximum(fk, np.concatenate([[0.0], fk[:-1]]))
    sl = PT.slack(q, sdot, vmax, amax, feed, pts, 0.5, k)
    assert (sl <= 64 * EPS + 2 * near).all(), float((sl - 2 * near).max())


@pytest.mark.parametrize("feed", [None, FEED])                             # varies fastest: both cases share their inputs
@pytest.mark.parametrize("name,nj", ROBOTS)
@pytest.mark.parametrize("G,R,N", SHAPES)
def test_every_path_keeps_the_contract(gpu, name, nj, feed, G, R, N):
    paths, state, want = _inputs(gpu, name, nj, G, R, N, seed=7 * N + G + R)
    vmax, amax = _limits(nj)
    k = 8 if N == 17 else 0
    timer = gpu.PathTimer(gpu.robotproperty2(name), vmax, amax, feed=feed, stops=k or "ends")
    r = timer.time(paths, state)
    np.testing.assert_array_equal(r.status, want)
    off = r.status != 0
    assert np.isnan(r.time[off]).all() and np.isnan(r.sdot[off]).all() and np.isnan(r.duration[off]).all()
    assert np.isfinite(r.time[~off]).all() and np.isfinite(r.sdot[~off]).all()
    # the selection against an argmin of the device's own durations, to the last bit
    sel, gs = PT.select(r.duration, r.status)
    np.testing.assert_array_equal(r.selected, sel)
    np.testing.assert_array_equal(r.group_status, gs)
    rows = [i for i in list(range(min(24, G * R))) + [G * R - 1] if not off.reshape(-1)[i]]
    q = paths.reshape(G * R, N, nj)[rows]
    pts = _points(gpu, name, nj, q) if feed else [None] * len(rows)
    tm, sd, du = r.time.reshape(G * R, N)[rows], r.sdot.reshape(G * R, N)[rows], r.duration.reshape(-1)[rows]
    for j in range(len(rows)):
        _check_path(q[j], tm[j], sd[j], du[j], vmax, amax, np.inf if feed is None else feed, pts[j], k)
    # doubling vmax and the feed and quadrupling amax halves every time stamp bit for bit
    fast = gpu.PathTimer(gpu.robotproperty2(name), 2 * vmax, 4 * amax, feed=None if feed is None else 2 * feed, stops=k or "ends").time(paths, state)
    np.testing.assert_array_equal(fast.status, r.status)
    np.testing.assert_array_equal(fast.time, r.time / 2)
    np.testing.assert_array_equal(fast.sdot, r.sdot * 2)
    np.testing.assert_array_equal(fast.selected, r.selected)


def test_the_trapezoid_and_a_tie(gpu):
    """joint 0 of the 2L moves 17 rows 0.1 rad apart, joint 1 a hundredth of that: L/v + v/a of joint 0; four copies tie"""
    q = np.zeros((1, 4, 17, 2))
    q[..., 0] = 0.1 * np.arange(17)
    q[..., 1] = 0.001 * np.arange(17)
    v, a = 0.1 * np.sqrt(32.0), 0.4
    timer = gpu.PathTimer(gpu.robotproperty2("2L"), [v, 1.0], [a, 1.0])
    r = timer.time(q)
    assert (r.status == 0).all() and (np.abs(r.duration - (1.6 / v + v / a)) <= 1e-12).all()
    assert r.selected[0] == 0 and (r.duration == r.duration[0, 0]).all()
    r = timer.time(q, state=np.array([[1, 0, 0, 0]]))
    assert r.selected[0] == 1 and r.status[0].tolist() == [1, 0, 0, 0]
    r = timer.time(q, state=np.ones((1, 4), int))
    assert r.selected[0] == -1 and r.group_status[0] == 1 and np.isnan(r.duration).all()


def test_stalled_paths(gpu):
    """stops every 2 rows on 4 rows: rows 2 and 3 both rest"""
    paths, _, _ = _inputs(gpu, "M200i", 5, 1, 3, 4, seed=2)
    r = gpu.PathTimer(gpu.robotproperty2("M200i"), 1.0, 2.0, stops=2).time(paths)
    assert (r.status == 3).all() and np.isnan(r.time).all() and np.isnan(r.sdot).all() and r.selected[0] == -1
    r = gpu.PathTimer(gpu.robotproperty2("M200i"), 1.0, 2.0, stops=3).time(paths)
    assert (r.status == 0).all() and (r.sdot[..., 0] == 0).all() and (r.sdot[..., 3] == 0).all() and (r.sdot[..., 1:3] > 0).all()


@pytest.mark.parametrize("name,nj", ROBOTS)
@pytest.mark.parametrize("with_feed", [False, True])
def test_parity_with_the_cpu_restatement(gpu, O, name, nj, with_feed):
    """status and selected equal; time stamps and sdot within max(1000 x the movement of the restatement's own answer under a 1e-12 rad
    change of every row, 1e-10): the rule of the Cartesian paths"""
    import ik_reference as R
    arm = R.Arm(O.robotproperty2(name), nj)
    lim = gpu.robotproperty2(name).thetamax[:nj]
    P = PT.PARITY
    for k in (0, 4):
        paths, _, out = PT.parity_case(arm, lim, k)
        ref, movement, tol = out[with_feed]
        timer = gpu.PathTimer(gpu.robotproperty2(name), P["vmax"], P["amax"], feed=P["feed"] if with_feed else None, curve_share=P["gamma"],
                              stops=k or "ends")
        got = timer.time(paths)
        np.testing.assert_array_equal(got.status, ref.status)
        np.testing.assert_array_equal(got.selected, ref.selected)
        np.testing.assert_array_equal(got.group_status, ref.group_status)
        dt, ds = np.abs(got.time - ref.time).max(), np.abs(got.sdot - ref.sdot).max()
        print(f"[path timing parity] {name} feed={with_feed} k={k}: |time - ref| <= {dt:.3e} s, |sdot - ref| <= {ds:.3e} (movement {movement:.3e}, "
              f"tolerance {tol:.3e})")
        assert dt <= tol and ds <= tol
        if not with_feed:                                                   # no forward kinematics: the same IEEE operations
            np.testing.assert_array_equal(got.time, ref.time)
            np.testing.assert_array_equal(got.sdot, ref.sdot)


def test_results_do_not_depend_on_the_batch_and_are_deterministic(gpu):
    import torch
    paths, state, _ = _inputs(gpu, "M200i", 5, 130, 64, 17, seed=5)
    vmax, amax = _limits(5)
    timer = gpu.PathTimer(gpu.robotproperty2("M200i"), vmax, amax, feed=FEED, stops=8)
    names = ("time", "sdot", "duration", "status", "selected", "group_status")
    big, again = timer.time(paths, state), timer.time(paths, state)
    for n in names:
        np.testing.assert_array_equal(getattr(big, n), getattr(again, n), err_msg=n)
    for rows in ([129], [5, 129, 64], [0]):                                  # alone, in a batch of 3 (other positions), first
        part = timer.time(paths[rows], state[rows])
        for n in names:
            np.testing.assert_array_equal(getattr(part, n), getattr(big, n)[rows], err_msg=n)
    lone = timer.time(paths[7, 9:12], state[7, 9:12])                        # three paths of a group as three groups of one
    for n in names[:4]:
        np.testing.assert_array_equal(getattr(lone, n), getattr(big, n)[7, 9:12], err_msg=n)
    assert (lone.selected == np.where(lone.status == 0, 0, -1)).all()
    # device tensors on a side stream behind other work, no host synchronisation in between
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    pd, sd = torch.tensor(paths, dtype=torch.float64, device=dev), torch.tensor(state, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        busy = torch.ones(2048, 2048, dtype=torch.float64, device=dev)
        for _ in range(4):
            busy = busy @ busy * 1e-4
        got = gpu.PathTimer(gpu.robotproperty2("M200i"), vmax, amax, feed=FEED, stops=8, device=dev).time_device(pd, sd, stream=side)
    side.synchronize()
    for n in names:
        np.testing.assert_array_equal(getattr(got, n).cpu().numpy(), getattr(big, n), err_msg=n)


def test_corners_on_the_candidates_of_a_followed_path(gpu):
    """cand_path and cand_status of a follow_device call go in as they are"""
    import torch
    from test_gpu_cart import _obstacles
    from test_gpu_cart_follow import _case
    Ks = 4
    lim, start, pos, axs, tref = _case(gpu, "M200i", 5, 3, 64, 3, True, seed=61)
    dev = torch.device("cuda", 0)
    d = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    robot = gpu.robotproperty2("M200i")
    fo = gpu.CartesianPath(robot, _obstacles(), steps=Ks, device=dev).follow_device(d(start), d(pos), d(axs), d(tref), want_candidates=True)
    timer = gpu.PathTimer(robot, 1.0, 2.0, feed=0.1, stops="corners", device=dev)
    r = timer.time_device(fo.cand_path, state=fo.cand_status, steps=Ks)
    torch.cuda.synchronize()
    cs, st, sd, du = fo.cand_status.cpu().numpy(), r.status.cpu().numpy(), r.sdot.cpu().numpy(), r.duration.cpu().numpy()
    assert tuple(r.time.shape) == (3, 64, 2 * Ks + 1) and (cs == 0).any() and (cs != 0).any()
    assert ((st == 1) == (cs != 0)).all() and np.isin(st[cs == 0], (0, 4)).all() and (st == 0).any()
    assert np.isnan(sd[st != 0]).all() and np.isnan(du[st != 0]).all()
    t = sd[st == 0]
    assert (t[:, ::Ks] == 0.0).all() and (np.delete(t, np.arange(0, 2 * Ks + 1, Ks), axis=1) > 0).all()
    sel, gs = PT.select(du, st)
    np.testing.assert_array_equal(r.selected.cpu().numpy(), sel)
    np.testing.assert_array_equal(r.group_status.cpu().numpy(), gs)
    host = gpu.PathTimer(robot, 1.0, 2.0, feed=0.1, stops="corners").time(fo.cand_path.cpu().numpy(), fo.cand_status.cpu().numpy(), steps=Ks)
    np.testing.assert_array_equal(host.time, r.time.cpu().numpy())
    np.testing.assert_array_equal(host.selected, sel)
    print(f"[path timing] {int((st == 0).sum())} of {st.size} candidates timed; the soonest takes {np.nanmin(du):.3f} s, follow's own winner "
          f"{[float(du[g, s]) if s >= 0 else None for g, s in enumerate(fo.selected.cpu().numpy())]}")


def test_plan_to_path_with_path_timing(gpu):
    import torch
    from test_gpu_cart_follow import _ell
    pobs, s, g, region_g, region_s, off = gpu.RRTstar_problem()
    S, Ks = 4, 4
    planner = gpu.RRTCFSPlanner(pobs, s, region_g, region_s, off, num_seed=2, max_slots=S)
    lim = s.robot.thetamax[:5]
    rng = np.random.default_rng(71)
    goals = []
    obs6, D = gpu.obs_to_array(pobs), np.array([o["D"] for o in pobs])
    while len(goals) < S:                                                    # first configurations that RRT's feasible() accepts
        gq = np.asarray(s.goal_th) + 0.15 * (2 * rng.random(5) - 1)
        dd, _ = gpu.dist_arm(s.robot, gq[None], obs6)
        if ((dd[0] - D) >= 0.02).all() and (gq > lim[:, 0]).all() and (gq < lim[:, 1]).all():
            goals.append(gq)
    pos, axs = _ell(gpu, np.array(goals), 0.04, 0.04)
    pos[1] += np.array([50.0, 0.0, 0.0])                                     # slot 1: no IK solution (-2)
    x0 = np.broadcast_to(np.asarray(s.x0, float), (S, 5)).copy()
    timing = dict(vmax=1.0, amax=2.0, feed=0.05, stops="corners")
    plain = planner.plan_to_path(x0, pos, axs, seed=3, path_steps=Ks)
    timed = planner.plan_to_path(x0, pos, axs, seed=3, path_steps=Ks, path_timing=timing)
    new = ("tool_path_time", "tool_path_sdot", "tool_path_duration", "tool_path_time_status")
    assert not any(hasattr(plain, n) for n in new)
    for n, v in vars(plain).items():                                         # nothing else changes, field for field
        if isinstance(v, torch.Tensor):
            x, y = v.cpu().numpy(), getattr(timed, n).cpu().numpy()
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), n
    assert set(vars(timed)) == set(vars(plain)) | set(new)
    # the manual composition: the winners' paths and their status into a PathTimer of the planner's device
    timer = gpu.PathTimer(s.robot, njoint=5, device=planner.device, **timing)
    want = timer.time_device(timed.tool_path, state=timed.tool_path_status, steps=Ks)
    torch.cuda.synchronize()
    for n, w in zip(new, (want.time, want.sdot, want.duration, want.status)):
        x, y = getattr(timed, n).cpu().numpy(), w.cpu().numpy()
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), n
    ok = (timed.tool_path_status == 0).cpu().numpy()
    st, du, tm = timed.tool_path_time_status.cpu().numpy(), timed.tool_path_duration.cpu().numpy(), timed.tool_path_time.cpu().numpy()
    assert tuple(timed.tool_path_time.shape) == (S, 2 * Ks + 1) and ok.any() and timed.status[1] == -2
    assert (st[~ok] == 1).all() and np.isnan(du[~ok]).all() and np.isnan(tm[~ok]).all()
    assert np.isin(st[ok], (0, 4)).all() and (st[ok] == 0).any() and (du[st == 0] > 0).all()
    # -3: no joint may move, so no candidate follows the path
    none = planner.plan_to_path(x0, pos, axs, seed=3, path_steps=Ks, path_options=dict(max_joint_step=1e-5), path_timing=timing)
    assert (none.status[[0, 2, 3]] == -3).all() and (none.tool_path_time_status == 1).all() and torch.isnan(none.tool_path_time).all()
    # plan_to_pose: the approach line of 5 cm under a feed of 5 cm/s takes a second at the least
    tp, ta = gpu.tool_pose(s.robot, np.array(goals))
    back, K, feed = 0.05, 8, 0.05
    ap = planner.plan_to_pose(x0, tp, ta, seed=3, approach=back, approach_steps=K, approach_timing=dict(vmax=1.0, amax=2.0, feed=feed))
    bare = planner.plan_to_pose(x0, tp, ta, seed=3, approach=back, approach_steps=K)
    new = ("approach_time", "approach_sdot", "approach_duration", "approach_time_status")
    assert set(vars(ap)) == set(vars(bare)) | set(new)
    for n, v in vars(bare).items():
        if isinstance(v, torch.Tensor):
            x, y = v.cpu().numpy(), getattr(ap, n).cpu().numpy()
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), n
    want = gpu.PathTimer(s.robot, 1.0, 2.0, feed=feed, njoint=5, device=planner.device).time_device(ap.approach_path, state=ap.approach_status)
    torch.cuda.synchronize()
    for n, w in zip(new, (want.time, want.sdot, want.duration, want.status)):
        x, y = getattr(ap, n).cpu().numpy(), w.cpu().numpy()
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), n
    st, du = ap.approach_time_status.cpu().numpy(), ap.approach_duration.cpu().numpy()
    assert tuple(ap.approach_time.shape) == (S, K + 1) and ((st == 0) == (ap.approach_status.cpu().numpy() == 0)).all() and (st == 0).any()
    assert (du[st == 0] >= (back - K * 2e-6) / feed).all()                   # the chords between rows that are on the line to tol_pos = 1e-6
    planner.close()
