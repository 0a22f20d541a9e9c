"""Clearance audit with moving meshes (cfs_clearance_mesh_motion_device) on config 5 and on config 5 with a
carrier travelling through the cell (workloads.config5_traveller).  Oracle-free.
For CFS and PSGCFS on each workload, three states of one handle: static meshes (audited by cfs_clearance_mesh_device: the
baseline), identity poses and the workload's own poses (both audited by the new entry; identity poses run the posed kernels over
held intervals and must give the static audit's bits).  Per state: one batched solve, then the audit of its outputs with S = 4,
16, 64 sub-steps per interval: the audit's time (device events around the call on one stream, W warm-up calls, median / min / max
of R timed ones, device-resident inputs, the pose table already built by the warm-up calls) next to the solve's, and of the
plans with status 0/1 the share that is more than 1 cm short of its margin at a waypoint / along the path, with the lowest
distances and the worst dist_path - dist_lower.

    python tools/clearance_motion_ab.py [--batch B] [--repeats R] [--warmup W] [--json profiles/clearance_motion_ab.json]
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
from clearance_mesh_ab import timed  # noqa: E402

OUT = ("dist_wp", "dist_path", "dist_lower", "t_path", "link_path", "tri_path")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)  # noqa: E731
    s5, bt5, tri5 = workloads.config5(B=a.batch)
    sT, btT, trisT, posesT = workloads.config5_traveller(B=a.batch)
    loads = {"config5": (s5, bt5, [tri5], None), "config5_traveller": (sT, btT, trisT, posesT)}
    rows = []
    for name, (s, bt, tris, poses) in loads.items():
        meshes = [pkg.Mesh(tri=x) for x in tris]
        eye = [np.eye(4)] * len(tris)
        states = [("static", None), ("identity", eye)] + ([("moving", list(poses))] if poses is not None else [])
        for mode in ("CFS", "PSGCFS"):
            psg = mode == "PSGCFS"
            margin = bt.margin_psg if psg else bt.margin_cfs
            h = pkg.CFSBatch(s, bt.nobs, margin, mode=mode, max_batch=bt.B)
            h.set_meshes(meshes)
            args = [t(bt.x_init), t(bt.xR1), t(bt.ff), t(bt.caug), t(bt.obs)]
            nz = t(bt.noise) if psg else None
            out, buf = h.alloc_outputs(bt.B, dev), h.alloc_clearance_mesh(bt.B, dev)
            static = {}
            for state, P in states:
                h.set_mesh_motion(P)
                entry = h.clearance_mesh_device if P is None else h.clearance_mesh_motion_device
                solve_ms = timed(lambda: h.solve_device(*args, noise=nz, out=out), 1, 3)
                st = out.status.cpu().numpy()
                ok = st <= 1
                row = dict(workload=name, mode=mode, state=state, B=bt.B, triangles=[int(x.shape[0]) for x in tris], H=int(s.H),
                           status=np.bincount(st, minlength=5).tolist(), solved=int(ok.sum()), solve_ms=solve_ms[0],
                           solve_ms_min=solve_ms[1], solve_ms_max=solve_ms[2], audit={})
                audit = lambda S: entry(out.x_, out.u, args[1], args[4], substeps=S, out=buf)  # noqa: E731
                audit(64)                              # the workspace and the table grow once, outside the timed calls
                for S in (4, 16, 64):
                    ms = timed(lambda: audit(S), a.warmup, a.repeats)
                    rec = dict(ms=ms[0], ms_min=ms[1], ms_max=ms[2], ms_over_solve=ms[0] / solve_ms[0])
                    got = {k: getattr(buf, k).cpu().numpy().copy() for k in OUT}
                    wp, path, low = (got[k][ok] for k in ("dist_wp", "dist_path", "dist_lower"))
                    if ok.any():
                        rec.update(short_wp=float((wp < margin - 0.01).any(axis=1).mean()), short_path=float((path < margin - 0.01).any(axis=1).mean()),
                                   min_wp=float(wp.min()), min_path=float(path.min()), worst_gap=float((path - low).max()),
                                   worst_dip=float((wp - path).max()))
                    if state == "static":
                        static[S] = got
                    elif state == "identity":
                        rec["bitwise_static"] = all((got[k] == static[S][k]).all() for k in OUT)
                    row["audit"][S] = rec
                rows.append(row)
                print(json.dumps(row), flush=True)
            h.close()
        for m in meshes:
            m.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
