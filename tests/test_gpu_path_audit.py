"""Tool-path audit on the GPU (cfs_path_audit*, PathAudit.audit / audit_device, the planner's path_audit / approach_audit) against the
properties the contract promises, checked on the device's own output with tests/path_audit_reference.py's checkers, and against the
CPU restatement.

Shapes: G = 1, 3, 130 x R = 64, 7, 1 x N = 2 (one segment), 3, 17, 257 x S = 1 (the rows alone), 3, 64 -- every value of every axis at
least once, not their product; 257 rows x 64 sub-steps (16 385 samples, 261 passes of the wavefront) on one path only; 130 x 64 paths
are 8 320 workgroups.  A pass holds 63 sub-intervals: (N, S) = (17, 3) is 48 of them (below a wavefront), (2, 64) 64 (one above), (3, 64)
two full passes and two left over, (2, 1) and (3, 1) one and two.  M200i (5 joints), M16iB (6), 2L (2) and the M200i's first 3 and 4
joints, so all five instantiations run.  Paths are straight joint moves plus a sine term; every fifth path has a state != 0, path 1
a NaN row; two line obstacles.  The per-path properties are checked on the first paths of a batch and on its last, the batch-wide
ones (statuses, NaN rows, state_out) on all."""
import functools

import numpy as np
import pytest

import path_audit_reference as PA

pytestmark = pytest.mark.gpu

ROBOTS = [("M200i", 5), ("M16iB", 6), ("2L", 2)]
CASES = [  # name, nj, G, R, N, S
    ("M200i", 5, 1, 64, 2, 1), ("M200i", 5, 3, 7, 3, 3), ("M200i", 5, 130, 64, 17, 3), ("M200i", 5, 1, 1, 257, 64), ("M200i", 5, 130, 1, 2, 64),
    ("M16iB", 6, 3, 64, 3, 64), ("M16iB", 6, 1, 7, 17, 1), ("2L", 2, 130, 7, 3, 1), ("2L", 2, 3, 1, 17, 64),
    ("M200i", 3, 3, 7, 17, 3), ("M200i", 4, 1, 64, 3, 64),
]


def _arm(O, name, nj):
    import ik_reference as IR
    return IR.Arm(O.robotproperty2(name), nj)


def _lim(pkg, name, nj):
    return np.asarray(pkg.robotproperty2(name).thetamax[:nj], float)


def _cell(obs, D):
    return [dict(l=np.stack([o[:3], o[3:]], axis=1), D=float(d)) for o, d in zip(obs, D)]


@functools.lru_cache(maxsize=4)
def _inputs(name, nj, G, R, N, seed):
    """paths (G, R, N, nj), state (G, R); made once for the cases that share them and left unchanged"""
    import motionplanning_5d_m_amd as pkg
    return PA.parity_inputs(_lim(pkg, name, nj), G, R, N, seed)


def _ns(r):
    """numpy namespace of a result of audit() or audit_device()"""
    from types import SimpleNamespace
    return SimpleNamespace(**{k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in vars(r).items()})


@pytest.mark.parametrize("name,nj,G,R,N,S", CASES)
def test_every_path_keeps_the_contract(gpu, O, name, nj, G, R, N, S):
    arm, lim = _arm(O, name, nj), _lim(gpu, name, nj)
    paths, state = _inputs(name, nj, G, R, N, 7 * N + G + R)
    obs, D = PA.two_obstacles(arm, lim)
    robot = gpu.robotproperty2(name)
    finite = np.isfinite(paths).all(axis=(2, 3))
    free = gpu.PathAudit(robot, _cell(obs, D), njoint=nj).audit(paths, state, substeps=S)
    PA.check_conventions(free, state, finite)
    PA.check_state_out(free)
    np.testing.assert_array_equal(free.state_out[finite], state[finite])     # thresholds off: state_out == state on finite paths
    ok = free.status == 0
    # thresholds at the medians of the device's own bounds: both decisions occur, and each follows from the path's own outputs
    mc, xc = float(np.median(free.clear_lower[ok])), float(np.median(free.chord_upper[ok]))
    thr = gpu.PathAudit(robot, _cell(obs, D), njoint=nj, min_clearance=mc, max_chord=xc).audit(paths, state, substeps=S)
    PA.check_conventions(thr, state, finite)
    PA.check_state_out(thr, mc, xc)
    for k in PA.FLOATS + ("link_path", "obs_path", "status"):
        np.testing.assert_array_equal(getattr(thr, k), getattr(free, k), err_msg=k)   # the thresholds change state_out alone
    none = gpu.PathAudit(robot, None, njoint=nj).audit(paths, state, substeps=S)
    PA.check_conventions(none, state, finite)
    np.testing.assert_array_equal(none.chord_err, free.chord_err)
    np.testing.assert_array_equal(none.chord_upper, free.chord_upper)
    flat = paths.reshape(G * R, N, nj)
    rows = [i for i in list(range(min(6, G * R))) + [G * R - 1] if ok.reshape(-1)[i]]
    for i in rows:
        r = PA.pick(free, i)
        PA.check_path(arm.robot, nj, arm.tool, flat[i], S, len(D), r)
        PA.check_path(arm.robot, nj, arm.tool, flat[i], S, 0, PA.pick(none, i))
        if (N - 1) * S * 16 <= 4096:                                         # the 16 times denser sampling on the CPU
            PA.check_sound(arm, flat[i], obs, D, S, r)


@pytest.mark.parametrize("name,nj", ROBOTS + [("M200i", 3), ("M200i", 4)])
def test_parity_with_the_cpu_restatement(gpu, O, name, nj):
    """status, state_out, link_path and obs_path equal; every float within max(1000 x the movement of the restatement's own answer under
    a 1e-12 rad change of every row, 1e-10); s_path equal where the first minimum is separated from the runner-up by more than that:
    the rule of the Cartesian paths"""
    arm, lim = _arm(O, name, nj), _lim(gpu, name, nj)
    paths, state, obs, D, mc, xc, ref, movement, tol = PA.parity_case(arm, lim)
    G, R = state.shape
    got = gpu.PathAudit(gpu.robotproperty2(name), _cell(obs, D), njoint=nj, min_clearance=mc, max_chord=xc).audit(paths, state, substeps=PA.PARITY["S"])
    ok = ref.status.reshape(G, R) == 0
    for k in PA.INTS:
        np.testing.assert_array_equal(getattr(got, k), getattr(ref, k).reshape(G, R), err_msg=k)
    sep = ok & (ref.gap.reshape(G, R) > tol["clear_path"])
    np.testing.assert_array_equal(got.s_path[sep], ref.s_path.reshape(G, R)[sep])
    diffs = {}
    for k in PA.FLOATS:
        if k != "s_path":
            diffs[k] = float(np.abs(getattr(got, k)[ok] - getattr(ref, k).reshape(G, R)[ok]).max())
    print(f"[path audit parity] {name} nj={nj}: " + ", ".join(f"|{k} - ref| <= {v:.2e} (tol {tol[k]:.2e})" for k, v in diffs.items())
          + f"; s_path compared on {int(sep.sum())} of {int(ok.sum())}")
    for k, v in diffs.items():
        assert v <= tol[k], (k, v, tol[k])


@pytest.mark.parametrize("name,nj", ROBOTS)
def test_the_post_between_two_rows(gpu, O, name, nj):
    arm = _arm(O, name, nj)
    q, obs, D = PA.post_scene(arm)
    a = gpu.PathAudit(gpu.robotproperty2(name), _cell(obs, D), njoint=nj, min_clearance=0.0)
    out = {S: a.audit(q, substeps=S) for S in (2, 3, 8)}
    print(f"[path audit post, device] {name}: rows clear by {float(out[2].clear_rows):.3f} m; clear_path "
          + ", ".join(f"S={S}: {float(r.clear_path):+.3f}" for S, r in out.items()) + "; clear_lower "
          + ", ".join(f"S={S}: {float(r.clear_lower):+.3f}" for S, r in out.items()))
    for S, r in out.items():
        assert r.status == 0 and r.clear_rows > 0 and r.clear_lower < 0 and r.state_out == 6 and r.obs_path == 0
        want = PA.audit_path(arm, q, obs, D, S, min_clearance=0.0)
        assert r.link_path == want.link_path and r.s_path == want.s_path
        assert abs(float(r.clear_path) - want.clear_path) <= 1e-9 and abs(float(r.clear_lower) - want.clear_lower) <= 1e-9
    assert out[2].clear_path < 0 and out[8].clear_path < 0 and out[2].s_path == 0.5 and out[8].s_path == 0.5 and out[3].clear_path > 0


def test_results_do_not_depend_on_the_batch_and_are_deterministic(gpu, O):
    import torch
    name, nj, G, R, N, S = "M200i", 5, 130, 64, 17, 3
    arm, lim = _arm(O, name, nj), _lim(gpu, name, nj)
    paths, state = _inputs(name, nj, G, R, N, 7 * N + G + R)
    obs, D = PA.two_obstacles(arm, lim)
    robot = gpu.robotproperty2(name)
    audit = gpu.PathAudit(robot, _cell(obs, D), min_clearance=0.01, max_chord=5e-3)
    names = PA.FLOATS + PA.INTS
    big, again = audit.audit(paths, state, substeps=S), audit.audit(paths, state, substeps=S)
    for n in names:
        np.testing.assert_array_equal(getattr(big, n), getattr(again, n), err_msg=n)
    for rows in ([129], [5, 129, 64], [0]):                                  # alone, in a batch of 3 (other positions), first
        part = audit.audit(paths[rows], state[rows], substeps=S)
        for n in names:
            np.testing.assert_array_equal(getattr(part, n), getattr(big, n)[rows], err_msg=n)
    lone = audit.audit(paths[7, 9:12], state[7, 9:12], substeps=S)           # three paths of a group as three groups of one
    one = audit.audit(paths[7, 10], substeps=S)                              # a single path, no state
    for n in names:
        np.testing.assert_array_equal(getattr(lone, n), getattr(big, n)[7, 9:12], err_msg=n)
        np.testing.assert_array_equal(getattr(one, n), getattr(big, n)[7, 10], err_msg=n)
    # device tensors on a side stream behind other work, no host synchronisation in between
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    pd, sd = torch.tensor(paths, dtype=torch.float64, device=dev), torch.tensor(state, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        busy = torch.ones(2048, 2048, dtype=torch.float64, device=dev)
        for _ in range(4):
            busy = busy @ busy * 1e-4
        got = gpu.PathAudit(robot, _cell(obs, D), min_clearance=0.01, max_chord=5e-3, device=dev).audit_device(pd, sd, substeps=S, stream=side)
    side.synchronize()
    for n in names:
        np.testing.assert_array_equal(getattr(got, n).cpu().numpy(), getattr(big, n), err_msg=n)


def test_followed_candidates_their_clearance_and_the_timer_behind_the_audit(gpu):
    """cand_path and cand_status of a follow_device call go in as they are; clear_rows of a winner is follow's clearance as the header
    states it (to the parity tolerance, not promised to the last bit); state_out goes into PathTimer as it is"""
    import torch
    from test_gpu_cart import _obstacles
    from test_gpu_cart_follow import _case
    Ks = 4
    lim, start, pos, axs, tref = _case(gpu, "M200i", 5, 3, 64, 3, True, seed=61)
    dev = torch.device("cuda", 0)
    d = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    robot = gpu.robotproperty2("M200i")
    fo = gpu.CartesianPath(robot, _obstacles(), steps=Ks, device=dev).follow_device(d(start), d(pos), d(axs), d(tref), want_candidates=True)
    free = gpu.PathAudit(robot, _obstacles(), device=dev).audit_device(fo.cand_path, state=fo.cand_status, substeps=8)
    torch.cuda.synchronize()
    cs, sel, clr = fo.cand_status.cpu().numpy(), fo.selected.cpu().numpy(), fo.clearance.cpu().numpy()
    f = _ns(free)
    assert tuple(free.clear_path.shape) == (3, 64) and (cs == 0).any() and (cs != 0).any() and (sel >= 0).any()
    assert ((f.status == 1) == (cs != 0)).all() and (f.status[cs == 0] == 0).all()
    np.testing.assert_array_equal(f.state_out, cs)                           # thresholds off
    won = [g for g in range(3) if sel[g] >= 0]
    rows = np.array([f.clear_rows[g, sel[g]] for g in won])
    print(f"[path audit] clear_rows of {len(won)} follow winners against follow's clearance: largest difference "
          f"{np.abs(rows - clr[won]).max():.3e} m ({'equal' if (rows == clr[won]).all() else 'not equal'} bit for bit)")
    assert (np.abs(rows - clr[won]) <= 1e-10).all()
    assert (f.clear_rows[cs == 0] >= 0).all()                                # a complete candidate collides at no row
    # thresholds at the medians of the audited candidates: the timer then selects among those that pass only
    ok = cs == 0
    mc, xc = float(np.median(f.clear_lower[ok])), float(np.median(f.chord_upper[ok]))
    au = gpu.PathAudit(robot, _obstacles(), device=dev, min_clearance=mc, max_chord=xc).audit_device(fo.cand_path, state=fo.cand_status, substeps=8)
    timer = gpu.PathTimer(robot, 1.0, 2.0, feed=0.1, device=dev)
    tm, all_ = timer.time_device(fo.cand_path, state=au.state_out), timer.time_device(fo.cand_path, state=fo.cand_status)
    torch.cuda.synchronize()
    a, t = _ns(au), _ns(tm)
    PA.check_state_out(a, mc, xc)
    assert np.isin(a.state_out[ok], (0, 6, 7)).all() and (a.state_out[ok] == 6).any() and (a.state_out[ok] == 0).any()
    assert ((t.status == 1) == (a.state_out != 0)).all()
    for g in range(3):
        if t.selected[g] >= 0:
            assert a.state_out[g, t.selected[g]] == 0
            passing = (a.state_out[g] == 0) & (t.status[g] == 0)
            assert t.duration[g, t.selected[g]] == t.duration[g][passing].min()
        else:
            assert not ((a.state_out[g] == 0) & (_ns(all_).status[g] == 0)).any()
    assert (t.selected >= 0).any()
    host = gpu.PathAudit(robot, _obstacles(), min_clearance=mc, max_chord=xc).audit(fo.cand_path.cpu().numpy(), fo.cand_status.cpu().numpy(), substeps=8)
    for n in PA.FLOATS + PA.INTS:
        np.testing.assert_array_equal(getattr(host, n), getattr(a, n), err_msg=n)


# ---- the planner ------------------------------------------------------------------------------------------------------------------------
def _same(a, b, names=None):
    import torch
    for n, v in vars(a).items():
        if isinstance(v, torch.Tensor) and (names is None or n in names):
            x, y = v.cpu().numpy(), getattr(b, n).cpu().numpy()
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), n


def test_the_planner_takes_the_nearest_candidate_that_passes(gpu):
    """plan_to_path(path_audit=) on 4 slots: slot 1 has no IK solution (-2); across the second segment of slot 2's path, between rows
    Ks+1 and Ks+2, stands a post 2 mm thick: every row of every candidate clears it by 4 mm (follow completes), every candidate's
    tool point goes through it between the two rows (-4).  Against the manual composition IK -> follow -> audit -> argmin, and field
    for field against the unaudited call when the thresholds are off.  plan_to_pose(approach_audit=) the same way."""
    import torch
    from test_gpu_cart_follow import _ell
    pobs, s, g, region_g, region_s, off = gpu.RRTstar_problem()
    S, Ks, side = 4, 4, 0.04
    lim = s.robot.thetamax[:5]
    rng = np.random.default_rng(71)
    goals = []
    obs6, D = gpu.obs_to_array(pobs), np.array([o["D"] for o in pobs])
    while len(goals) < S:                                                    # first configurations that RRT's feasible() accepts
        gq = np.asarray(s.goal_th) + 0.15 * (2 * rng.random(5) - 1)
        dd, _ = gpu.dist_arm(s.robot, gq[None], obs6)
        if ((dd[0] - D) >= 0.02).all() and (gq > lim[:, 0]).all() and (gq < lim[:, 1]).all():
            goals.append(gq)
    pos, axs = _ell(gpu, np.array(goals), 0.04, side)
    pos[1] += np.array([50.0, 0.0, 0.0])                                     # slot 1: no IK solution (-2)
    a, e = axs[2, 0], (pos[2, 2] - pos[2, 1]) / side
    mid = pos[2, 1] + 0.015 * e                                              # rows Ks+1 and Ks+2 stand at 0.010 and 0.020 along e
    cell = list(pobs) + [dict(shape="cylinder", l=np.stack([mid - 0.03 * a, mid + 0.03 * a], axis=1), D=0.001, epsilon=0.001)]
    planner = gpu.RRTCFSPlanner(cell, s, region_g, region_s, off, num_seed=2, max_slots=S)
    dev = planner.device
    x0 = np.broadcast_to(np.asarray(s.x0, float), (S, 5)).copy()
    new = ("tool_path_clear_lower", "tool_path_clear_path", "tool_path_chord_err", "tool_path_chord_upper", "tool_path_audit_state")
    plain = planner.plan_to_path(x0, pos, axs, seed=3, path_steps=Ks)
    free = planner.plan_to_path(x0, pos, axs, seed=3, path_steps=Ks, path_audit={})
    assert not any(hasattr(plain, n) for n in new) and set(vars(free)) == set(vars(plain)) | set(new)
    _same(plain, free)                                                       # thresholds off: nothing else changes, field for field
    aud = planner.plan_to_path(x0, pos, axs, seed=3, path_steps=Ks, path_audit=dict(substeps=8, min_clearance=0.0))
    st, fst = aud.status.cpu().numpy(), plain.tool_path_status.cpu().numpy()
    assert fst[2] == 0 and fst[0] == 0 and fst[3] == 0 and fst[1] != 0        # follow completes on slot 2: its rows clear the post
    assert st[1] == -2 and st[2] == -4 and st[0] not in (-2, -3, -4) and st[3] not in (-2, -3, -4), st
    assert aud.has_solution[2] == 0 and aud.selected[2] == -1 and aud.tool_path_audit_state[2] == 6 and aud.tool_path_clear_lower[2] < 0
    assert (aud.tool_path_audit_state[[0, 3]] == 0).all() and (aud.tool_path_clear_lower[[0, 3]] >= 0).all()
    # the manual composition
    d = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)  # noqa: E731
    robot = s.robot
    sol = gpu.IKSolver(robot, cell, njoint=5, device=dev).solve_device(d(pos[:, 0]), d(axs[:, 0]), d(x0), seed=3, want_candidates=True)
    fo = gpu.CartesianPath(robot, cell, njoint=5, device=dev, steps=Ks).follow_device(sol.cand_theta, d(pos), d(axs), d(x0), start_state=sol.cand_status,
                                                                                      want_candidates=True)
    au = gpu.PathAudit(robot, cell, njoint=5, device=dev, min_clearance=0.0).audit_device(fo.cand_path, state=fo.cand_status, substeps=8)
    torch.cuda.synchronize()
    dl = sol.cand_theta - d(x0)[:, None, :]
    cost = torch.zeros_like(au.clear_lower)
    for c in range(5):
        cost = cost + dl[:, :, c] * dl[:, :, c]
    passing = (au.state_out == 0).cpu().numpy()
    cost = np.where(passing, cost.cpu().numpy(), np.inf)
    idx, passed = cost.argmin(axis=1), passing.any(axis=1)
    np.testing.assert_array_equal(passed, [True, False, False, True])
    assert (fo.cand_status[2] == 0).any() and not passing[2].any()           # -4: complete candidates, none passes
    cp, sel = fo.cand_path.cpu().numpy(), aud.tool_path_selected.cpu().numpy()
    for k in (0, 3):
        assert sel[k] == idx[k]
        np.testing.assert_array_equal(aud.tool_path[k].cpu().numpy(), cp[k, idx[k]])
        np.testing.assert_array_equal(aud.goal[k].cpu().numpy(), cp[k, idx[k], 0])
        for n in new[:4]:
            assert getattr(aud, n)[k] == getattr(au, n[len("tool_path_"):])[k, idx[k]], n
    np.testing.assert_array_equal(aud.tool_path[2].cpu().numpy(), plain.tool_path[2].cpu().numpy())   # the path that failed stays visible
    # the fields are the audit of the path reported
    again = gpu.PathAudit(robot, cell, njoint=5, device=dev, min_clearance=0.0).audit_device(aud.tool_path, state=aud.tool_path_status, substeps=8)
    torch.cuda.synchronize()
    for n in new[:4]:
        x, y = getattr(aud, n).cpu().numpy(), getattr(again, n[len("tool_path_"):]).cpu().numpy()
        assert np.array_equal(x[[0, 2, 3]], y[[0, 2, 3]]) and np.isnan(x[1]), n
    # plan_to_pose: the approach line
    tp, ta = gpu.tool_pose(robot, np.array(goals))
    tp[1] += np.array([50.0, 0.0, 0.0])
    new = ("approach_clear_lower", "approach_clear_path", "approach_chord_err", "approach_chord_upper", "approach_audit_state")
    bare = planner.plan_to_pose(x0, tp, ta, seed=3, approach=0.05, approach_steps=8)
    free = planner.plan_to_pose(x0, tp, ta, seed=3, approach=0.05, approach_steps=8, approach_audit={})
    assert set(vars(free)) == set(vars(bare)) | set(new)
    _same(bare, free)
    ap = planner.plan_to_pose(x0, tp, ta, seed=3, approach=0.05, approach_steps=8, approach_audit=dict(substeps=4, max_chord=1e-9))
    ok = (bare.approach_status == 0).cpu().numpy()
    assert ok.any() and ap.status[1] == -2
    assert (ap.status.cpu().numpy()[ok] == -4).all() and (ap.approach_audit_state.cpu().numpy()[ok] == 7).all()   # no joint-linear chord is that exact
    again = gpu.PathAudit(robot, cell, njoint=5, device=dev, max_chord=1e-9).audit_device(ap.approach_path, state=ap.approach_status, substeps=4)
    torch.cuda.synchronize()
    for n in new[:4]:
        x, y = getattr(ap, n).cpu().numpy(), getattr(again, n[len("approach_"):]).cpu().numpy()
        assert np.array_equal(x[ok], y[ok]) and (x[ok] == x[ok]).all(), n
    planner.close()
