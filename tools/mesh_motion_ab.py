"""A/B of moving meshes (cfs_problem_set_mesh_motion) on config 5.  Oracle-free.
For CFS and PSGCFS, three cases:
  static      config 5: the assembly-line map, the default handle                    (workloads.config5)
  identity    the same handle shape with identity poses set                          (bit for bit `static`: checked here)
  traveller   the map held still plus a carrier riding the conveyor, nmesh = 2        (workloads.config5_traveller)
Reported per (mode, case): ms per batched solve (median and min-max over `rounds` rounds of K timed solves after W warm-up ones,
the cases alternating round by round on one stream, device-resident inputs), outer iterations per second, statuses.

    python tools/mesh_motion_ab.py [--batch B] [--steps K] [--warmup W] [--rounds R] [--json profiles/mesh_motion_ab.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import motionplanning_5d_m_amd as pkg  # noqa: E402
from motionplanning_5d_m_amd import workloads  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)  # noqa: E731
    s, bt, tri = workloads.config5(B=a.batch)
    st, btt, tris, poses = workloads.config5_traveller(B=a.batch)
    m_map, m_car = pkg.Mesh(tri=tri), pkg.Mesh(tri=tris[1])
    rows = []
    for mode in ("CFS", "PSGCFS"):
        psg = mode == "PSGCFS"
        cases = {
            "static": (s, bt, [m_map], None),
            "identity": (s, bt, [m_map], np.eye(4)[None]),
            "traveller": (st, btt, [m_map, m_car], poses),
        }
        run = {}
        for name, (fam, b, meshes, P) in cases.items():
            h = pkg.CFSBatch(fam, b.nobs, b.margin_psg if psg else b.margin_cfs, mode=mode, max_batch=b.B)
            h.set_meshes(meshes)
            if P is not None:
                h.set_mesh_motion(P)
            args = [t(b.x_init), t(b.xR1), t(b.ff), t(b.caug), t(b.obs)]
            nz = t(b.noise) if psg else None
            out = h.alloc_outputs(b.B, dev)
            for _ in range(a.warmup):
                h.solve_device(*args, noise=nz, out=out)
            torch.cuda.synchronize()
            run[name] = (h, args, nz, out, [])
        for _ in range(a.rounds):
            for name, (h, args, nz, out, ms) in run.items():
                for _ in range(a.steps):
                    t0 = time.perf_counter()
                    h.solve_device(*args, noise=nz, out=out)
                    torch.cuda.synchronize()
                    ms.append((time.perf_counter() - t0) * 1e3)
        fields = ("u", "x_", "cost_all", "e_cost_all", "e_u_all", "iter_O", "total_iter", "status")
        ref = {f: getattr(run["static"][3], f).cpu().numpy() for f in fields}
        for name, (h, args, nz, out, ms) in run.items():
            stt = out.status.cpu().numpy()
            n_it = int((out.iter_O.cpu().numpy() - 1).sum())
            med = float(np.median(ms))
            row = dict(mode=mode, case=name, B=a.batch, nmesh=len(cases[name][2]), ms_per_solve=med, ms_min=float(np.min(ms)),
                       ms_max=float(np.max(ms)), solves=len(ms), outer_it=n_it, outer_it_per_s=n_it / med * 1e3,
                       status=np.bincount(stt, minlength=5).tolist())
            if name == "identity":
                row["bitwise_equal_to_static"] = all(np.array_equal(getattr(out, f).cpu().numpy(), ref[f]) for f in ref)
            rows.append(row)
            print(json.dumps(row), flush=True)
            h.close()
        base = next(r["ms_per_solve"] for r in rows if r["mode"] == mode and r["case"] == "static")
        for r in rows:
            if r["mode"] == mode:
                r["ms_vs_static"] = r["ms_per_solve"] / base
        print(json.dumps({"mode": mode, "ms_vs_static": {r["case"]: round(r["ms_vs_static"], 4) for r in rows if r["mode"] == mode}}),
              flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
