"""A/B of joint position limits (cfs_problem_set_joint_limits) on config 3.  Oracle-free.
For CFS and PSGCFS, three cases on the same batch:
  unlimited   the default handle
  never       a handle limited to +-1e6 rad on every joint: rows that never bind   (bit for bit `unlimited`: checked here)
  cell        a handle limited to workloads.CONFIG3_CELL_LIMITS, which bind
Reported per (mode, case): ms per batched solve (median over `rounds` rounds of K timed solves after W warm-up ones, the cases
alternating round by round on one stream, device-resident inputs), outer iterations per second, statuses.

    python tools/limits_ab.py [--batch B] [--steps K] [--warmup W] [--rounds R] [--json out.json]
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
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    t = lambda x: torch.tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)  # noqa: E731
    dist = lambda rb, th, ob: pkg.dist_arm(rb, th, ob)[0]  # noqa: E731
    s, bt = workloads.config3(dist, B=a.batch)
    never = np.array([[-1e6, 1e6]] * 5)
    rows = []
    for mode in ("CFS", "PSGCFS"):
        psg = mode == "PSGCFS"
        cases = {"unlimited": None, "never": never, "cell": workloads.CONFIG3_CELL_LIMITS}
        run = {}
        for name, lim in cases.items():
            b = bt
            h = pkg.CFSBatch(s, b.nobs, b.margin_psg if psg else b.margin_cfs, mode=mode, max_batch=b.B, joint_limits=lim)
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
        ref = {f: getattr(run["unlimited"][3], f).cpu().numpy() for f in ("u", "x_", "iter_O", "total_iter", "status")}
        for name, (h, args, nz, out, ms) in run.items():
            st = out.status.cpu().numpy()
            n_it = int((out.iter_O.cpu().numpy() - 1).sum())
            med = float(np.median(ms))
            row = dict(mode=mode, case=name, B=a.batch, ms_per_solve=med, ms_min=float(np.min(ms)), ms_max=float(np.max(ms)),
                       solves=len(ms), outer_it=n_it, outer_it_per_s=n_it / med * 1e3, status=np.bincount(st, minlength=5).tolist())
            if name == "never":
                row["bitwise_equal_to_unlimited"] = all(np.array_equal(getattr(out, f).cpu().numpy(), ref[f]) for f in ref)
            rows.append(row)
            print(json.dumps(row), flush=True)
            h.close()
        base = next(r["ms_per_solve"] for r in rows if r["mode"] == mode and r["case"] == "unlimited")
        for r in rows:
            if r["mode"] == mode:
                r["ms_vs_unlimited"] = r["ms_per_solve"] / base
        print(json.dumps({"mode": mode, "ms_vs_unlimited": {r["case"]: round(r["ms_vs_unlimited"], 4) for r in rows if r["mode"] == mode}}),
              flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
