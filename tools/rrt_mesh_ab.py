"""RRT trees against mesh obstacles (cfs_rrt_grow_mesh_device) on the reference-map workload
(workloads.rrt_reference_map: the assembly-line cell, 13 258 triangles, D = 0.2).  Oracle-free.

grow:    trees/s of one launch of N trees (N = 1024, 4096) for variant A (per lane) and variant B (wave-cooperative), and for
         the same starts / goals / seed with the mesh removed (the line-only kernel through cfs_rrt_grow_device, no obstacle left).
         The three are timed ALTERNATELY in one process: R rounds of (A, B, none), one launch each between two events; median,
         min and max per variant.  A and B must give identical trees (checked).  ns per proposal = launch time / proposals.
planner: RRTCFSPlanner end to end on S slots, num_seed = 6, per mode (CFS, PSGCFS): the grow / build / solve / audit / select
         split of timings=, the share of slots with a solution, and the final cost of the kept plans next to the same solver
         started from the straight joint-space line (what config5_reference_map runs), same horizon and cost family as the planner's.

    python tools/rrt_mesh_ab.py [--trees 1024 4096] [--rounds R] [--slots S] [--json profiles/rrt_mesh_ab.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import motionplanning_5d_m_amd as pkg  # noqa: E402
from motionplanning_5d_m_amd import workloads  # noqa: E402
from motionplanning_5d_m_amd.sysinfo import cost_terms  # noqa: E402

FIELDS = ("node_num", "fail", "route_len", "parent", "nodes", "total_dis", "route", "proposals")


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def stats(ms):
    return dict(ms=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)))


def grow_ab(N, rounds, seed, dev):
    w = workloads.rrt_reference_map(S=N)
    mesh = pkg.Mesh(tri=w.tri)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)  # noqa: E731
    x0, goal = t(w.x0), t(w.goal)
    with_mesh = pkg.RRT_FANUC(w.obs_cell(mesh), w.sys_rrt, w.sys_rrt.goal_th, w.region_g, w.region_s, w.sample_off, "M200i", "RRT")
    without = pkg.RRT_FANUC([], w.sys_rrt, w.sys_rrt.goal_th, w.region_g, w.region_s, w.sample_off, "M200i", "RRT")
    runs = {"A_per_lane": lambda: with_mesh.grow_device(N, seed, dev, x0=x0, goal=goal, want_tree=True, mesh_flags=1),
            "B_wave": lambda: with_mesh.grow_device(N, seed, dev, x0=x0, goal=goal, want_tree=True, mesh_flags=2),
            "no_mesh": lambda: without.grow_device(N, seed, dev, x0=x0, goal=goal, want_tree=True)}
    ms, last = {k: [] for k in runs}, {}
    for k, fn in runs.items():                               # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in runs.items():
            m, last[k] = once(fn)
            ms[k].append(m)
    same = all(torch.equal(getattr(last["A_per_lane"], f), getattr(last["B_wave"], f)) for f in FIELDS)
    row = dict(part="grow", trees=N, triangles=int(w.tri.shape[0]), rounds=rounds, seed=seed, A_equals_B=bool(same), variants={})
    for k in runs:
        r = last[k]
        props, nodes = int(r.proposals.sum().item()), int(r.node_num.sum().item())
        st = stats(ms[k])
        row["variants"][k] = dict(**st, trees_per_s=N / (st["ms"] * 1e-3), proposals=props, nodes=nodes, found=int((r.fail == 0).sum().item()),
                                  ns_per_proposal=st["ms"] * 1e6 / max(props, 1))
    mesh.close()
    return row


def planner_rows(S, seed, dev):
    w = workloads.rrt_reference_map(S=S)
    mesh = pkg.Mesh(tri=w.tri)
    rows = []
    for mode in ("CFS", "PSGCFS"):
        pl = pkg.RRTCFSPlanner(w.obs_cell(mesh), w.sys_rrt, w.region_g, w.region_s, w.sample_off, num_seed=6, mode=mode, max_slots=S,
                               min_clearance=0.01)
        pl.plan(w.x0, w.goal, seed=seed)                     # warm-up
        tm = {}
        res = pl.plan(w.x0, w.goal, seed=seed, timings=tm)
        torch.cuda.synchronize()
        has = res.has_solution.cpu().numpy() != 0
        cost = res.cost.cpu().numpy()
        # the same solver from the straight line: the planner's own handle (same family, margins, mesh), one problem per slot
        s, nj, H = pl.sys_cfs, 5, pl.sys_cfs.H
        th = np.linspace(w.x0, w.goal, H + 1)[1:].transpose(1, 0, 2)
        x_init = np.concatenate([th, np.zeros_like(th)], axis=2).reshape(S, -1)
        xR1 = np.concatenate([w.x0, np.zeros((S, nj))], axis=1)
        ff, caug = np.zeros((S, H * nj)), np.zeros(S)
        for b in range(S):
            ff[b], caug[b] = cost_terms(s.Aaug, s.Baug, s.Qaug_state, xR1[b], w.goal[b], H, nj)
        t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)  # noqa: E731
        line = pl.cfs.solve_device(t(x_init), t(xR1), t(ff), t(caug), pl._obs[:S].contiguous())
        torch.cuda.synchronize()
        lst, lit = line.status.cpu().numpy(), line.iter_O.cpu().numpy()
        lcost = line.cost_all.cpu().numpy()[np.arange(S), np.maximum(lit - 2, 0)]
        lok = lst <= 1
        both = has & lok
        rows.append(dict(part="planner", mode=mode, slots=S, num_seed=6, seed=seed, timings_ms=tm, rounds_max=int(res.rounds.max().item()),
                         share_with_solution=float(has.mean()), share_clearance_ok=float((res.clearance_ok.cpu().numpy() != 0).mean()),
                         status=np.bincount(np.maximum(res.status.cpu().numpy(), 0), minlength=5).tolist(),
                         no_route=int((res.selected.cpu().numpy() < 0).sum()),
                         cost_median_rrt=float(np.median(cost[has])) if has.any() else None,
                         line_share_solved=float(lok.mean()), line_status=np.bincount(lst, minlength=5).tolist(),
                         cost_median_line=float(np.median(lcost[lok])) if lok.any() else None,
                         both=int(both.sum()), rrt_cheaper_share=float((cost[both] < lcost[both]).mean()) if both.any() else None,
                         cost_ratio_median_rrt_over_line=float(np.median(cost[both] / lcost[both])) if both.any() else None))
        pl.close()
    mesh.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, nargs="*", default=[1024, 4096])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []
    for N in a.trees:
        rows.append(grow_ab(N, a.rounds, a.seed, dev))
        print(json.dumps(rows[-1]), flush=True)
    if a.slots > 0:
        for r in planner_rows(a.slots, a.seed, dev):
            rows.append(r)
            print(json.dumps(r), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
