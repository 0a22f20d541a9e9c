"""Batched straight-line tool paths (cfs_cart_path_device) on the M200i.  Oracle-free.
T grasp targets (poses of seeded random configurations inside the joint ranges, made with cfs_tool_pose), an approach of `--approach`
metres along the tool axis, RRTstar_CFS.m's two line obstacles: one IK launch at the pre-grasp poses with R restarts, then the trace
from all T x R candidates in K steps.  Recorded: the trace's launch time (device events around the call on one stream, W warm-up
calls, median of N timed ones, device-resident inputs), the shares of candidate states, the targets solved, the largest per-lane
cand_iter and the time per pass (launch time / largest cand_iter).  Then RRTCFSPlanner on RRTstar_problem, 64 slots: plan_to_pose
with and without approach -- the IK, trace, grow and solve times, how many slots kept IK's own winner, how many switched candidate,
how many ended -3.

    python tools/cart_ab.py [--targets T] [--restarts R] [--steps K] [--approach M] [--repeats N] [--warmup W] [--json out.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import motionplanning_5d_m_amd as pkg  # noqa: E402
from ik_ab import configs, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=1024)
    ap.add_argument("--restarts", type=int, default=64)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--approach", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)  # noqa: E731
    pobs, s, g, region_g, region_s, off = pkg.RRTstar_problem()
    lines = [dict(l=o["l"], D=o["D"]) for o in pobs]
    robot, lim = s.robot, s.robot.thetamax[:5]
    q = configs(lim, a.targets, seed=1)
    pos, axis = pkg.tool_pose(robot, q)
    tref = configs(lim, a.targets, seed=2)
    ik = pkg.IKSolver(robot, lines, restarts=a.restarts, device=dev)
    cart = pkg.CartesianPath(robot, lines, steps=a.steps, device=dev)
    tp, ta, tr = t(pos), t(axis), t(tref)
    sol = ik.solve_device(t(pos - a.approach * axis), ta, tr, seed=7, want_candidates=True)
    torch.cuda.synchronize()
    run = lambda: cart.trace_device(sol.cand_theta, tp, ta, tr, start_state=sol.cand_status, want_candidates=True)  # noqa: E731
    ms = timed(run, a.warmup, a.repeats)
    r = run()
    torch.cuda.synchronize()
    cs, it, st = r.cand_status.cpu().numpy(), r.cand_iter.cpu().numpy(), r.status.cpu().numpy()
    started = cs != 5
    row = dict(robot="M200i", targets=a.targets, candidates=a.restarts, steps=a.steps, approach_m=a.approach, max_iter=cart.max_iter,
               max_joint_step=cart.max_joint_step, tol_pos=cart.tol_pos, tol_axis=cart.tol_axis, launch_ms_median=ms[0], launch_ms_min=ms[1],
               launch_ms_max=ms[2], ik_targets_solved=float((sol.status == 0).float().mean().item()),
               candidate_states={name: float((cs == k).mean()) for k, name in pkg._lib.CART_CAND_STATUS.items()},
               started_states={name: float((cs[started] == k).mean()) for k, name in pkg._lib.CART_CAND_STATUS.items()} if started.any() else None,
               targets_solved=float((st == 0).mean()), targets_no_line=float((st == 1).mean()), targets_no_start=float((st == 2).mean()),
               kept_ik_winner=int(((r.selected == sol.selected) & (r.status == 0)).sum().item()),
               switched_candidate=int(((r.selected != sol.selected) & (r.status == 0)).sum().item()),
               cand_iter_max=int(it.max()), cand_iter_mean_started=float(it[started].mean()) if started.any() else None,
               iterations_per_step_complete=float(it[cs == 0].mean() / a.steps) if (cs == 0).any() else None,
               us_per_pass=1e3 * ms[0] / max(1, int(it.max())))
    print(json.dumps(row))
    # the planner: grasp targets near the checked-in goal, 64 slots, with and without the approach
    S = 64
    planner = pkg.RRTCFSPlanner(pobs, s, region_g, region_s, off, max_slots=S)
    rng = np.random.default_rng(3)
    goals = np.asarray(s.goal_th)[None, :] + 0.15 * (2 * rng.random((S, 5)) - 1)
    gp, ga = pkg.tool_pose(robot, goals)
    x0 = t(np.broadcast_to(np.asarray(s.x0, float), (S, 5)))
    gtp, gta = t(gp), t(ga)
    kw = dict(approach=a.approach, approach_steps=a.steps)
    planner.plan_to_pose(x0, gtp, gta, seed=5, **kw)                    # warm-up
    planner.plan_to_pose(x0, gtp, gta, seed=5)
    pik = next(v for k, v in planner._ik.items() if k[:1] != ("approach",))
    pcart = next(v for k, v in planner._ik.items() if k[:1] == ("approach",))
    un = gta / torch.linalg.norm(gta, dim=1, keepdim=True)
    pre = (gtp - a.approach * un).contiguous()
    ik_ms = timed(lambda: pik.solve_device(pre, gta, x0, seed=5, want_candidates=True), a.warmup, a.repeats)
    psol = pik.solve_device(pre, gta, x0, seed=5, want_candidates=True)
    tr_ms = timed(lambda: pcart.trace_device(psol.cand_theta, gtp, gta, x0, start_state=psol.cand_status), a.warmup, a.repeats)
    tm_app, tm_plain = {}, {}
    res = planner.plan_to_pose(x0, gtp, gta, seed=5, timings=tm_app, **kw)
    plain = planner.plan_to_pose(x0, gtp, gta, seed=5, timings=tm_plain)
    torch.cuda.synchronize()
    ok = res.approach_status == 0
    plan_row = dict(slots=S, num_seed=planner.K, approach_m=a.approach, steps=a.steps, ik_solved=int((res.ik_status == 0).sum().item()),
                    approach_solved=int(ok.sum().item()), kept_ik_winner=int((ok & (res.approach_selected == psol.selected)).sum().item()),
                    switched_candidate=int((ok & (res.approach_selected != psol.selected)).sum().item()),
                    ended_minus_3=int((res.status == -3).sum().item()), ended_minus_2=int((res.status == -2).sum().item()),
                    has_solution=int(res.has_solution.sum().item()), plain_has_solution=int(plain.has_solution.sum().item()),
                    ik_launch_ms_median=ik_ms[0], trace_launch_ms_median=tr_ms[0], with_approach_parts_ms=tm_app, without_approach_parts_ms=tm_plain)
    print(json.dumps(plan_row))
    planner.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(tool="tools/cart_ab.py", device=torch.cuda.get_device_name(0), warmup=a.warmup, repeats=a.repeats, trace=row, planner=plan_row),
                      f, indent=1)


if __name__ == "__main__":
    main()
