"""A/B of the two Jacobian modes (fd_literal = num_jac.m literally, analytic = cfs_problem_set_jacobian(CFS_JAC_ANALYTIC)) on
BASELINE config 3 (workloads.config3, batch 1024), both solvers.  Oracle-free.  For each (solver, mode):
  * ms per solve and outer iterations per second: K solves of the resident batch on one handle and one stream, timed with
    HIP events around the timed block as bench.py's per-launch events are (after W warm-up solves);
  * the cycle stamps of the linearisation phase (cfs_debug_stamps, thread 0 of each workgroup; a separate solve): the share
    of workgroup time in sincos + kinematic chains (stamp 10), base distances (0), shifted-pose pairs | minima + tangents (11);
  * iteration counts and statuses.

    python tools/jacobian_ab.py [--steps K] [--warmup W] [--json out.json]
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

# stamp slots of cfs_solve_fused_kernel (tools/stamp_probe.py): 10 sincos + chains, 0 base distances (+ the literal scheme's
# minima / differences) and everything up to the QP, 11 segment pairs of the shifted poses | minima + tangent sweeps
LIN = {"sincos+chains": 10, "base dist (+rest)": 0, "shifted pairs | tangents": 11}


def run(s, bt, mode, jac, steps, warmup):
    B = bt.x_init.shape[0]
    margin = bt.margin_cfs if mode == "CFS" else bt.margin_psg
    slv = pkg.CFSBatch(s, bt.nobs, margin, mode=mode, max_batch=B, jacobian=jac)
    dev = torch.device("cuda:0")
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev).contiguous()  # noqa: E731
    args = (t(bt.x_init), t(bt.xR1), t(bt.ff), t(bt.caug), t(bt.obs))
    noise = t(bt.noise) if (mode == "PSGCFS" and bt.noise is not None) else None
    out = slv.alloc_outputs(B, dev)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            slv.solve_device(*args, noise=noise, out=out, stream=stream.cuda_stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(steps):
            slv.solve_device(*args, noise=noise, out=out, stream=stream.cuda_stream)
        e1.record(stream)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    iters = int((out.iter_O.cpu().numpy() - 1).sum())
    status = out.status.cpu().numpy()
    slv.stamps(B)
    r = slv.solve(bt.x_init, bt.xR1, bt.ff, bt.caug, bt.obs, noise=bt.noise if mode == "PSGCFS" else None)
    st = slv.stamps().astype(np.float64)
    slv.close()
    ok = r.status < 2
    tot, tot_ok = st.sum(), st[ok].sum()
    res = dict(mode=mode, jacobian=jac, ms_per_solve=ms, outer_iters=iters, iters_per_s=iters / (ms * 1e-3),
               status_counts={pkg.STATUS[k]: int((status == k).sum()) for k in range(4)},
               qp_steps=int(r.total_iter.sum()),
               lin_share_all={k: float(st[:, v].sum() / tot) for k, v in LIN.items()},
               lin_share_solved={k: float(st[ok][:, v].sum() / tot_ok) for k, v in LIN.items()},
               lin_cycles_per_iter_solved=float(st[ok][:, list(LIN.values())].sum() / max(int((r.iter_O[ok] - 1).sum()), 1)))
    return res, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert pkg.device_count() >= 1, "needs a GPU"
    s, bt = workloads.config3(lambda rb, th, ob: pkg.dist_arm(rb, th, ob)[0], B=1024)
    out = []
    for mode in ("PSGCFS", "CFS"):
        rr = {}
        for jac in ("fd_literal", "analytic"):
            res, rr[jac] = run(s, bt, mode, jac, a.steps, a.warmup)
            out.append(res)
            print(json.dumps(res))
        lit, an = rr["fd_literal"], rr["analytic"]
        both = (lit.status < 2) & (an.status < 2)
        dx = np.abs(lit.x_ - an.x_).max(axis=1)[both]
        print(f"[{mode}] status agreement {(lit.status == an.status).mean():.4f}; |x_ analytic - x_ literal|_inf on {int(both.sum())} "
              f"OK in both: median {np.median(dx):.1e}, max {dx.max():.1e}; ms per solve {out[-2]['ms_per_solve']:.3f} -> "
              f"{out[-1]['ms_per_solve']:.3f}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
