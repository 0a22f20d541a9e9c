"""Tool paths (cfs_cart_follow_device) on the M200i against the straight line of cfs_cart_path_device at equal
rows.  Oracle-free.  Section 20's protocol: device events around the call on one stream, W warm-up calls, median of N timed ones,
device-resident inputs.  T grasp targets (poses of seeded random configurations inside the joint ranges, made with cfs_tool_pose), a
first pose `--approach` metres back along the tool axis, one IK launch there with R restarts, then from all T x R candidates:
  trace        cfs_cart_path_device, K = 16: the straight line from every candidate's own pose to the target (17 rows)
  follow_m2    cfs_cart_follow_device, M = 2, K = 16: the same line as the two-pose path [first pose, target] (the same 17 rows)
  follow_L     M = 3, K = 8: the line, then `--side` metres sideways (17 rows)
  follow_dense M = 17, K = 1: the line given as 17 poses (17 rows, every row a pose of the table)
with RRTstar_problem's two line obstacles, and each of the four again in the cell of tools/cart_mesh_ab.py's cylinder scene (the first
line obstacle and the 160-triangle cylinder; cfs_cart_path_mesh_device / cfs_cart_follow_mesh_device).  Reported per call: ms per
launch (median, min, max), the share of started candidates that complete, the iterations per row of the complete ones, the largest
per-lane cand_iter; and the ratio follow_m2 / trace of the medians, measured in the same run, next to the run-to-run spread of both.

    python tools/cart_follow_ab.py [--targets T] [--restarts R] [--approach M] [--side M] [--repeats N] [--warmup W] [--json out.json]
                                   [--lib NAME.so]
--lib: the build of the library to time (default libcfs_hip.so; a file next to it), for A/B runs against a build of another commit.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import motionplanning_5d_m_amd as pkg  # noqa: E402
from motionplanning_5d_m_amd import _lib  # noqa: E402
from ik_ab import configs, timed  # noqa: E402
import rrt_mesh_reference as M  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=1024)
    ap.add_argument("--restarts", type=int, default=64)
    ap.add_argument("--approach", type=float, default=0.1)
    ap.add_argument("--side", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "cart_follow_ab.json"))
    ap.add_argument("--lib", default="libcfs_hip.so")
    a = ap.parse_args()
    _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), a.lib)            # before the first lib() call
    dev = torch.device("cuda", 0)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)  # noqa: E731
    pobs, s, *_ = pkg.RRTstar_problem()
    robot, lim = s.robot, s.robot.thetamax[:5]
    pos, axis = pkg.tool_pose(robot, configs(lim, a.targets, seed=1))
    tref = t(configs(lim, a.targets, seed=2))
    pre = pos - a.approach * axis
    e = np.cross(axis, [0.0, 0.0, 1.0])
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    s16 = (np.arange(17) / 16.0)[None, :, None]
    paths = dict(follow_m2=(16, np.stack([pre, pos], axis=1)), follow_L=(8, np.stack([pre, pos, pos + a.side * e], axis=1)),
                 follow_dense=(1, pre[:, None, :] + s16 * (pos - pre)[:, None, :]))
    lines = [dict(l=o["l"], D=o["D"]) for o in pobs]
    scenes = [("lines", lines, None), ("cylinder", lines[:1], dict(mesh=pkg.Mesh(tri=M.scene_triangles()), D=M.CYL_D))]
    tp, ta = t(pos), t(axis)
    rows = []
    for scene, cell_lines, mesh in scenes:
        sol = pkg.IKSolver(robot, cell_lines, restarts=a.restarts, device=dev).solve_device(t(pre), ta, tref, seed=7, want_candidates=True)
        torch.cuda.synchronize()
        cell = cell_lines + ([mesh] if mesh else [])
        for name in ("trace", "follow_m2", "follow_L", "follow_dense"):
            K = 16 if name == "trace" else paths[name][0]
            cart = pkg.CartesianPath(robot, cell, steps=K, device=dev, meshes=mesh is not None)
            if name == "trace":
                Mp = 2
                run = lambda: cart.trace_device(sol.cand_theta, tp, ta, tref, start_state=sol.cand_status, want_candidates=True)  # noqa: E731
            else:
                pp = t(paths[name][1])
                Mp = pp.shape[1]
                pa = ta[:, None, :].expand(-1, Mp, -1).contiguous()
                run = lambda: cart.follow_device(sol.cand_theta, pp, pa, tref, start_state=sol.cand_status, want_candidates=True)  # noqa: E731
            ms = timed(run, a.warmup, a.repeats)
            r = run()
            torch.cuda.synchronize()
            cs, it, st = r.cand_status.cpu().numpy(), r.cand_iter.cpu().numpy(), r.status.cpu().numpy()
            N = r.cand_path.shape[2]
            started, done = cs != 5, cs == 0
            rows.append(dict(scene=scene, call=name, poses=Mp, steps=K, rows=N, targets=a.targets, candidates=a.restarts, launch_ms_median=ms[0],
                             launch_ms_min=ms[1], launch_ms_max=ms[2], started=float(started.mean()),
                             completed_of_started=float(done[started].mean()) if started.any() else None, targets_solved=float((st == 0).mean()),
                             iterations_per_row_complete=float(it[done].mean() / N) if done.any() else None, cand_iter_max=int(it.max()),
                             us_per_pass=1e3 * ms[0] / max(1, int(it.max()))))
            print(json.dumps(rows[-1]))
    ratios = {}
    for scene, _, _ in scenes:
        by = {r["call"]: r for r in rows if r["scene"] == scene}
        tr, fo = by["trace"], by["follow_m2"]
        ratios[scene] = dict(follow_m2_over_trace=fo["launch_ms_median"] / tr["launch_ms_median"],
                             trace_spread=(tr["launch_ms_max"] - tr["launch_ms_min"]) / tr["launch_ms_median"],
                             follow_m2_spread=(fo["launch_ms_max"] - fo["launch_ms_min"]) / fo["launch_ms_median"])
    print(json.dumps(ratios))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(tool="tools/cart_follow_ab.py", lib=a.lib, device=torch.cuda.get_device_name(0), warmup=a.warmup, repeats=a.repeats,
                           approach_m=a.approach, side_m=a.side, calls=rows, ratios=ratios), f, indent=1)


if __name__ == "__main__":
    main()
