"""select="shortest" (the reference's rule, s_Parallel_rrt.m:27-28) against select="best" (every seed smoothed, best
smoothed result kept; include/cfs_hip.h cfs_select_best_device) on RRTstar_problem(), K = 6 seeds per slot.

For S = 256 and 682 slots (1 536 and 4 092 trees) and for STOP and SOFTEN (mu = 1e4): the solved fraction (status 0/1, and
0/1/4), the median final cost of the status-0/1 slots, for "best" the fraction of all found routes whose own solve ends 0/1,
and ms per plan() call split into grow / build / solve / select (HIP events on the stream; median of --reps calls after one
warm-up).  No oracle.  One JSON line per configuration, then a markdown table.  usage: python tools/plan_ab.py [--slots 256 682] [--reps 3] [--seed 20261015]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import motionplanning_5d_m_amd as pkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--slots", type=int, nargs="+", default=[256, 682])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--seed", type=int, default=20261015)
a = ap.parse_args()

pobs, s_r, g, region_g, region_s, off = pkg.RRTstar_problem()
rows = []
for S in a.slots:
    for pol, kw in (("stop", {}), ("soften 1e4", dict(on_infeasible="soften", soft_weight=1e4))):
        for sel in ("shortest", "best"):
            pl = pkg.RRTCFSPlanner(pobs, s_r, region_g, region_s, off, num_seed=6, select=sel, max_slots=S, **kw)
            x0, goal = np.tile(s_r.x0, (S, 1)), np.tile(g, (S, 1))   # S slots of RRTstar_CFS.m's start and goal
            pl.plan(x0, goal, a.seed)                           # warm-up (first launches, allocator)
            torch.cuda.synchronize()
            parts, walls = [], []
            for rep in range(a.reps):
                t = {}
                t0 = time.perf_counter()
                r = pl.plan(x0, goal, a.seed + rep, timings=t, want_candidates=sel == "best")
                torch.cuda.synchronize()
                walls.append((time.perf_counter() - t0) * 1e3)
                parts.append(t)
            st, cost = r.status.cpu().numpy(), r.cost.cpu().numpy()
            ok = np.isin(st, (0, 1))
            res = {"slots": S, "trees": S * 6, "policy": pol, "select": sel, "solved_01": float(ok.mean()),
                   "solved_014": float(np.isin(st, (0, 1, 4)).mean()),
                   "median_cost_01": float(np.median(cost[ok])) if ok.any() else None,
                   "ms_plan": statistics.median(walls),
                   **{"ms_" + k: statistics.median(p[k] for p in parts) for k in ("grow", "build", "solve", "select")},
                   "rounds_max": int(r.rounds.max().item()), "seed_of_last_rep": a.seed + a.reps - 1}
            if sel == "best":                                   # per found route, as if every seed were smoothed alone
                c = r.candidates
                okc = c.route_ok.cpu().numpy() != 0
                res["candidates_solved_01"] = float(np.isin(c.status.cpu().numpy()[okc], (0, 1)).mean())
            print(json.dumps(res), flush=True)
            rows.append(res)
            pl.close()
print("| S | trees | policy | select | solved 0/1 | solved 0/1/4 | median cost 0/1 | ms plan | grow | build | solve | select |")
print("|---|---|---|---|---|---|---|---|---|---|---|---|")
for r in rows:
    mc = f"{r['median_cost_01']:.4g}" if r["median_cost_01"] is not None else "-"
    print(f"| {r['slots']} | {r['trees']} | {r['policy']} | {r['select']} | {r['solved_01']:.3f} | {r['solved_014']:.3f} | {mc} | "
          f"{r['ms_plan']:.1f} | {r['ms_grow']:.1f} | {r['ms_build']:.2f} | {r['ms_solve']:.1f} | {r['ms_select']:.3f} |")
