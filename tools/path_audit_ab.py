"""Tool-path audit (cfs_path_audit_device) on the M200i.  Oracle-free.  Section 20's protocol: device events around
the call on one stream, W warm-up calls, median of N timed ones, device-resident inputs.  G groups x R paths of N rows: straight joint
moves plus a sine term of at most 0.2 rad per row, made on the device (tools/path_time_ab.py's); every path is audited (no state), against
two line obstacles near the tool points of the middle of the joint ranges.  Cases: 1 024 x 64 paths of 17 rows -- every candidate of a
follow launch -- at S = 4, 8 and 16 sub-steps per segment.  Reported per case: ms per launch (median, min, max) of cfs_path_audit_device
itself on outputs allocated once, ms per call of PathAudit.audit_device, which also allocates and zero-fills its ten result tensors, the
samples per path and the ns per sample; next to them the follow launch that produces 1 024 x 64 x 17 rows, from
profiles/cart_follow_ab.json.  The recipe only: nothing here asserts a time.

    python tools/path_audit_ab.py [--groups G] [--repeats N] [--warmup W] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import motionplanning_5d_m_amd as pkg  # noqa: E402
from motionplanning_5d_m_amd import _args, _lib  # noqa: E402
from ik_ab import timed  # noqa: E402
from path_time_ab import smooth_paths  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "path_audit_ab.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    robot = pkg.robotproperty2("M200i")
    nj, R, N = 5, 64, 17
    lim = np.asarray(robot.thetamax[:nj], float)
    p = pkg.tool_pose(robot, 0.5 * (lim[:, 0] + lim[:, 1])[None, :], njoint=nj)[0][0]
    obs = [dict(l=np.stack([p + [0.3, -0.5, -0.2], p + [0.3, 0.5, 0.3]], axis=1), D=0.02),
           dict(l=np.stack([p + [-0.6, 0.4, 0.5], p + [-0.4, 0.5, -0.5]], axis=1), D=0.03)]
    paths = smooth_paths(torch.tensor(lim, dtype=torch.float64, device=dev), a.groups, R, N, seed=N + R, dev=dev)
    rows = []
    for S in (4, 8, 16):
        audit = pkg.PathAudit(robot, obs, min_clearance=0.0, max_chord=2e-3, device=dev)
        call = timed(lambda: audit.audit_device(paths, substeps=S), a.warmup, a.repeats)
        r = audit.audit_device(paths, substeps=S)              # its tensors are the preallocated outputs of the bare entry
        d, o = audit._desc(S, audit._dev[1], audit._dev[2]), _args.fill(_lib.cfs_audit_out(), r)
        args = (C.byref(d), a.groups, R, N, _args.ptr(paths), None, C.byref(o))
        entry = _lib.lib().cfs_path_audit_device

        def bare():
            _lib.check(entry(*args, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        ms = timed(bare, a.warmup, a.repeats)
        torch.cuda.synchronize()
        n, per = a.groups * R, (N - 1) * S + 1
        rows.append(dict(groups=a.groups, paths_per_group=R, rows=N, substeps=S, samples_per_path=per, launch_ms_median=ms[0], launch_ms_min=ms[1],
                         launch_ms_max=ms[2], call_ms_median=call[0], call_ms_min=call[1], call_ms_max=call[2], ns_per_sample=ms[0] * 1e6 / (n * per),
                         certified=float((r.clear_lower > 0).double().mean()), passing=float((r.state_out == 0).double().mean()),
                         chord_upper_median=float(r.chord_upper.median())))
        print(json.dumps(rows[-1]))
    follow = None
    prof = os.path.join(ROOT, "profiles", "cart_follow_ab.json")
    if os.path.exists(prof):
        by = {(c["scene"], c["call"]): c for c in json.load(open(prof))["calls"]}
        f = by[("lines", "follow_L")]
        follow = dict(call="follow_L", targets=f["targets"], candidates=f["candidates"], rows=f["rows"], launch_ms_median=f["launch_ms_median"],
                      launch_ms_min=f["launch_ms_min"], launch_ms_max=f["launch_ms_max"])
        print(json.dumps(follow))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(tool="tools/path_audit_ab.py", device=torch.cuda.get_device_name(0), warmup=a.warmup, repeats=a.repeats, cases=rows,
                           follow_launch=follow), f, indent=1)


if __name__ == "__main__":
    main()
