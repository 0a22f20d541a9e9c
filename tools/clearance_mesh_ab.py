"""Clearance audit with mesh obstacles (cfs_clearance_mesh_device) on config 5: the reference's own
assembly-line triangles (workloads.config5_reference_map) and the synthetic map (workloads.config5).  Oracle-free.
For CFS and PSGCFS on each workload: one batched solve, then the audit of its outputs with S = 4, 16, 64 sub-steps per interval.
Reported per (workload, mode): statuses; of the problems with status 0/1 the share that is more than 1 cm short of its margin at
a waypoint / along the path, the lowest dist_wp / dist_path, the worst dist_path - dist_lower per S; the audit's time per S next
to the solve's (device events around the call on one stream, W warm-up calls, median of R timed ones, device-resident inputs);
and at S = 16 the A/B of the query variants in this one process (cold, bounded, seeded, both), whose outputs must agree bit for bit.

    python tools/clearance_mesh_ab.py [--batch B] [--repeats R] [--warmup W] [--json profiles/clearance_mesh_ab.json]
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

VARIANTS = (("cold", dict(clear_no_bound=True)), ("bound", {}), ("seed", dict(clear_no_bound=True, clear_seed=True)),
            ("bound+seed", dict(clear_seed=True)))
OUT = ("dist_wp", "dist_path", "dist_lower", "t_path", "link_path")


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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)  # noqa: E731
    loads = {"config5_reference_map": workloads.config5_reference_map(B=a.batch), "config5": workloads.config5(B=a.batch)}
    rows = []
    for name, (s, bt, tri) in loads.items():
        mesh = pkg.Mesh(tri=tri)
        for mode in ("CFS", "PSGCFS"):
            psg = mode == "PSGCFS"
            margin = bt.margin_psg if psg else bt.margin_cfs
            h = pkg.CFSBatch(s, bt.nobs, margin, mode=mode, max_batch=bt.B)
            h.set_meshes([mesh])
            args = [t(bt.x_init), t(bt.xR1), t(bt.ff), t(bt.caug), t(bt.obs)]
            nz = t(bt.noise) if psg else None
            out = h.alloc_outputs(bt.B, dev)
            solve_ms = timed(lambda: h.solve_device(*args, noise=nz, out=out), 1, 3)
            st = out.status.cpu().numpy()
            ok = st <= 1
            row = dict(workload=name, mode=mode, B=bt.B, triangles=int(tri.shape[0]), H=int(s.H), status=np.bincount(st, minlength=5).tolist(),
                       solved=int(ok.sum()), solve_ms=solve_ms[0], solve_ms_min=solve_ms[1], solve_ms_max=solve_ms[2], audit={}, variants={})
            buf = h.alloc_clearance_mesh(bt.B, dev)
            audit = lambda S: h.clearance_mesh_device(out.x_, out.u, args[1], args[4], substeps=S, out=buf)  # noqa: E731
            audit(64)                                  # the workspace grows once, outside the timed calls
            for S in (4, 16, 64):
                ms = timed(lambda: audit(S), a.warmup, a.repeats)
                wp, path, low = (getattr(buf, k).cpu().numpy()[ok] for k in ("dist_wp", "dist_path", "dist_lower"))
                queries = bt.B * (s.H * S + 1) * 5 * 1
                row["audit"][S] = dict(ms=ms[0], ms_min=ms[1], ms_max=ms[2], ms_over_solve=ms[0] / solve_ms[0], link_queries=queries,
                                       ns_per_query=ms[0] * 1e6 / queries,
                                       short_wp=float((wp < margin - 0.01).any(axis=1).mean()) if ok.any() else None,
                                       short_path=float((path < margin - 0.01).any(axis=1).mean()) if ok.any() else None,
                                       min_wp=float(wp.min()) if ok.any() else None, min_path=float(path.min()) if ok.any() else None,
                                       worst_gap=float((path - low).max()) if ok.any() else None)
            ref = None
            for vname, flags in VARIANTS:              # one process, one handle, the same inputs
                h.debug_options(**flags)
                ms = timed(lambda: audit(16), a.warmup, a.repeats)
                got = {k: getattr(buf, k).cpu().numpy().copy() for k in OUT}
                ref = got if ref is None else ref
                row["variants"][vname] = dict(ms=ms[0], ms_min=ms[1], ms_max=ms[2], bitwise_cold=all((got[k] == ref[k]).all() for k in OUT))
            h.debug_options()
            rows.append(row)
            print(json.dumps(row), flush=True)
            h.close()
        mesh.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
