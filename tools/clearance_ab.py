"""Clearance audit (cfs_clearance_device) on config 3 and config3_moving.  Oracle-free.
For CFS and PSGCFS on each workload: one batched solve, then the audit of its outputs with S = 4, 16, 64 sub-steps per interval.
Reported per (workload, mode): statuses; of the problems with status 0/1 the share that is more than 1 cm short of its margin at
a waypoint / along the path, the lowest dist_wp / dist_path, the worst dist_path - dist_lower per S; the audit's time per S next
to the solve's (device events around the call on one stream, W warm-up calls, median of R timed ones, device-resident inputs).

    python tools/clearance_ab.py [--batch B] [--repeats R] [--warmup W] [--json out.json]
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


def timed(fn, warmup, repeats):
    """median / min / max milliseconds of fn() between two events on the current stream"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)  # noqa: E731
    dist = lambda rb, th, ob: pkg.dist_arm(rb, th, ob)[0]  # noqa: E731
    loads = {"config3": workloads.config3(dist, B=a.batch) + ("static",),
             "config3_moving": workloads.config3_moving(dist, B=a.batch) + ("per_waypoint",)}
    rows = []
    for name, (s, bt, motion) in loads.items():
        for mode in ("CFS", "PSGCFS"):
            psg = mode == "PSGCFS"
            margin = bt.margin_psg if psg else bt.margin_cfs
            h = pkg.CFSBatch(s, bt.nobs, margin, mode=mode, max_batch=bt.B, obstacles=motion)
            args = [t(bt.x_init), t(bt.xR1), t(bt.ff), t(bt.caug), t(bt.obs)]
            nz = t(bt.noise) if psg else None
            out = h.alloc_outputs(bt.B, dev)
            solve_ms = timed(lambda: h.solve_device(*args, noise=nz, out=out), a.warmup, max(a.repeats // 3, 3))
            st = out.status.cpu().numpy()
            ok = st <= 1
            row = dict(workload=name, mode=mode, B=bt.B, status=np.bincount(st, minlength=5).tolist(), solved=int(ok.sum()),
                       solve_ms=solve_ms[0], solve_ms_min=solve_ms[1], solve_ms_max=solve_ms[2], audit={})
            for S in (4, 16, 64):
                buf = h.alloc_clearance(bt.B, dev)
                ms = timed(lambda: h.clearance_device(out.x_, out.u, args[1], args[4], substeps=S, out=buf), a.warmup, a.repeats)
                wp, path, low = (getattr(buf, k).cpu().numpy()[ok] for k in ("dist_wp", "dist_path", "dist_lower"))
                row["audit"][S] = dict(ms=ms[0], ms_min=ms[1], ms_max=ms[2], ms_over_solve=ms[0] / solve_ms[0],
                                       short_wp=float((wp < margin - 0.01).any(axis=1).mean()),
                                       short_path=float((path < margin - 0.01).any(axis=1).mean()),
                                       min_wp=float(wp.min()), min_path=float(path.min()), worst_gap=float((path - low).max()),
                                       certified=float((low >= margin - 0.01).all(axis=1).mean()))
            rows.append(row)
            print(json.dumps(row), flush=True)
            h.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
