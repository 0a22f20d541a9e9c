"""Inverse kinematics against mesh obstacles (cfs_ik_solve_mesh_device) on the M200i: what the mesh test costs
inside the IK launch.  Oracle-free.  Section 20's protocol: device events around the call on one stream, W warm-up calls, median of N
timed ones, device-resident inputs.  T targets (poses of seeded random configurations inside the joint ranges, made with
cfs_tool_pose), R restarts each, with the tool axis, on two scenes:
  cylinder       RRTstar_problem's first line obstacle (D = 0.2) and the 160-triangle cylinder of tests/rrt_mesh_reference.py (D = 0.1)
  reference_map  the reference's assembly-line cell (tests/golden/assembly_line_cell.npz through workloads.rrt_reference_map, D = 0.2)
and per scene three launches: line-only (cfs_ik_solve_device on the scene's lines: the baseline), mesh variant A, mesh variant B.
Reported next to the times: the share of converged restarts and of targets that the meshes reject, the candidates whose frontier
overflowed (variant B), and whether A and B returned the same bits.

    python tools/ik_mesh_ab.py [--targets T] [--restarts R] [--repeats N] [--warmup W] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import motionplanning_5d_m_amd as pkg  # noqa: E402
from motionplanning_5d_m_amd import _lib, workloads  # noqa: E402
from ik_ab import configs, timed  # noqa: E402
import rrt_mesh_reference as M  # noqa: E402

OUT = ("theta", "status", "selected", "n_ok", "err_pos", "err_axis", "clearance", "cand_theta", "cand_status", "cand_iter")


def overflows(reset=False):
    n = C.c_ulonglong(0)
    _lib.check(_lib.lib().cfs_debug_ik_frontier_overflows(C.byref(n), 1 if reset else 0))
    return int(n.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=1024)
    ap.add_argument("--restarts", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)  # noqa: E731
    pobs, s, *_ = pkg.RRTstar_problem()
    robot, lim = s.robot, s.robot.thetamax[:5]
    pos, axis = pkg.tool_pose(robot, configs(lim, a.targets, seed=1))
    args = (t(pos), t(axis), t(configs(lim, a.targets, seed=2)))
    w = workloads.rrt_reference_map(S=64)
    scenes = [("cylinder", [pobs[0]], pkg.Mesh(tri=M.scene_triangles()), M.CYL_D), ("reference_map", [], pkg.Mesh(tri=w.tri), float(w.D))]
    rows = []
    for name, lines, mesh, D in scenes:
        got = {}
        for variant in (None, "per_lane", "wave"):
            cell = lines + ([dict(mesh=mesh, D=D)] if variant else [])
            slv = pkg.IKSolver(robot, cell, restarts=a.restarts, device=dev, mesh_variant=variant)
            ms = timed(lambda: slv.solve_device(*args, seed=7, want_candidates=True), a.warmup, a.repeats)
            overflows(reset=True)
            r = slv.solve_device(*args, seed=7, want_candidates=True)
            torch.cuda.synchronize()
            over = overflows()
            got[variant] = {k: getattr(r, k).cpu().numpy() for k in OUT}
            cs, st = got[variant]["cand_status"], got[variant]["status"]
            row = dict(scene=name, triangles=int(mesh.info()["ntri"]), variant={None: "line-only", "per_lane": "A", "wave": "B"}[variant],
                       targets=a.targets, restarts=a.restarts, launch_ms_median=ms[0], launch_ms_min=ms[1], launch_ms_max=ms[2],
                       restarts_free=float((cs == 0).mean()), restarts_in_collision=float((cs == 2).mean()), targets_solved=float((st == 0).mean()),
                       targets_all_colliding=float((st == 2).mean()), frontier_overflows=over)
            if variant:
                base = got[None]
                past_lines = base["cand_status"] == 0
                row.update(vs_line_only=ms[0] / rows_base_ms, mesh_tests=int(past_lines.sum()),
                           rejected_by_mesh_of_converged=float(((cs == 2) & past_lines).sum() / max(1, past_lines.sum())),
                           targets_rejected_by_mesh=float(((st == 2) & (base["status"] == 0)).mean()),
                           us_per_mesh_test=1e3 * (ms[0] - rows_base_ms) / max(1, past_lines.sum()))
            else:
                rows_base_ms = ms[0]
            rows.append(row)
            print(json.dumps(row))
        same = all(np.array_equal(got["per_lane"][k], got["wave"][k], equal_nan=True) for k in OUT)
        rows.append(dict(scene=name, a_and_b_bit_identical=bool(same)))
        print(json.dumps(rows[-1]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(tool="tools/ik_mesh_ab.py", device=torch.cuda.get_device_name(0), warmup=a.warmup, repeats=a.repeats, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
