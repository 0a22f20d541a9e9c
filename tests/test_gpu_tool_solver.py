"""cfs_ik.hip and cfs_cart.hip take the workgroup staging, the convergence test, the cost chain, the wave argmin, the
winner's mesh clearance and the mesh decision from one place each (csrc/cfs_ik_dev.h, csrc/cfs_mesh_hit_dev.h).
The statements are the ones that stood in both units, so every output must equal, bit for bit, what the kernels returned before.

The recordings tests/golden/tool_solver_*.npy were written by `tests/tools/record_tool_solver.py` with the library built from the
commit BEFORE the change; the inputs are recorded with them.  Comparisons are exact equality of the bytes of every output field of
the host-array entries (NaN rows of unsolved targets and of unfinished paths included), one record per target.  Cases, shapes and
flag settings: tests/tool_solver_cases.py.  The follow_* cases pin the polyline trace the same way: they were recorded with the library
built from the commit BEFORE the line and the polyline kernel became cfs_cart_kernel<NJ, POLY> (DESIGN.md sections 23 and 27)."""
import json
import os

import numpy as np
import pytest

import tool_solver_cases as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def recording(case, variant=None, inputs=False):
    return np.load(os.path.join(GOLDEN, W.golden_name(case, variant, inputs)))


@pytest.mark.gpu
@pytest.mark.parametrize("case,variant", W.RUNS)
def test_outputs_equal_the_recording(gpu, case, variant):
    rec, want = recording(case, inputs=True), recording(case, variant)
    T = W.CASES[case]["T"]
    assert rec.shape[0] == want.shape[0] == T
    if W.CASES[case].get("mesh"):
        W.overflows(gpu, case, reset=True)
    got = W.run(gpu, case, variant, rec)
    for k in W.out_fields(case):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        bad = np.nonzero((a.reshape(T, -1).view(np.uint8) != b.reshape(T, -1).view(np.uint8)).any(axis=1))[0]
        assert bad.size == 0, f"{case} {variant or 'default'}: {k} differs from the recording in targets {bad.tolist()}"
    if W.CASES[case].get("mesh"):                                                # the same poses took the overflow fallback
        with open(os.path.join(GOLDEN, W.OVERFLOWS)) as f:
            assert W.overflows(gpu, case) == json.load(f)[case][variant or "default"]


def test_recordings_reach_the_states():
    """what the cases were designed for (no device work: the recorded results)"""
    for case, variant in W.RUNS:
        c, want = W.CASES[case], recording(case, variant)
        have = set(np.unique(want["cand_status"]).tolist())
        assert variant == W.LINE or set(c["states"]) <= have, (case, variant, sorted(have))
        assert (want["status"] == 0).any(), (case, variant)                     # some target has a winner: the selection and its outputs
        if c["R"] < 64:                                                          # idle lanes never win
            assert (want["selected"] < c["R"]).all()
    with open(os.path.join(GOLDEN, W.OVERFLOWS)) as f:
        over = json.load(f)
    for case in (k for k, c in W.CASES.items() if c.get("mesh")):
        line, first = recording(case, W.LINE), recording(case, W.MESH_VARIANTS[0])
        for variant in W.MESH_VARIANTS[1:]:                                      # every flag setting returns the same bytes
            assert first.tobytes() == recording(case, variant).tobytes(), (case, variant)
        # the mesh decision ran and rejected: candidates that are free of the lines (state 0 without the mesh) end in state 2
        # with it and others stay free.  A winner's clearance never rises with the mesh; in the inverse-kinematics scene the mesh
        # lowers it (in the Cartesian scene the one target that keeps its winner is nearer to its line obstacle than to the cylinder)
        rejected = (line["cand_status"] == 0) & (first["cand_status"] == 2)
        assert rejected.any() and ((line["cand_status"] == 0) & (first["cand_status"] == 0)).any(), case
        both = (line["status"] == 0) & (first["status"] == 0) & (line["selected"] == first["selected"])
        assert both.any() and (first["clearance"][both] <= line["clearance"][both]).all(), case
        if W.CASES[case]["kind"] == "ik":
            assert (first["clearance"][both] < line["clearance"][both]).any(), case
        # variant A and the full frontier never overflow; the 8-entry frontier does, so variant A decided those poses
        assert over[case][W.LINE] == 0 and over[case]["default"] == 0 and over[case]["per_lane"] == 0 and over[case]["small_frontier"] > 0, over[case]
